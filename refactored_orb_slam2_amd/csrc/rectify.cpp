// rectify.cpp -- C ABI of stereo rectification (include/orbfe.h: orbfe_rectifier_*, orbfe_rectify_*): what
// Source/Examples/Stereo/stereo_euroc.cc does with cv::initUndistortRectifyMap (:108-111, once per eye) and cv::remap (:159-160,
// both images of every frame) before TrackStereo.  The float maps are built here, on the host, in double, once per camera; the
// fixed-point map (rectify_internal.h) is derived from them at create time and uploaded.  orbfe_rectify_image runs the per-pixel
// arithmetic on the CPU for calibration-time use and for tests; the batch entry point validates and launches rectify_kernels.hip.
// No CPU fallback: a host-only handle passed to the batch entry point is an error.
//
// No OpenCV exists where this library is built and tested: the map arithmetic is this project's reading of OpenCV 4.5's scalar
// paths, as unpinned as the other OpenCV primitives.
#include <math.h>

#include <algorithm>
#include <new>
#include <vector>

#include "rectify_internal.h"

void orbfe_set_error(const char* fmt, ...);

struct orbfe_rectifier {
  orbfe_rectify_camera cam{};
  int device = -1;                      // -1: host-only
  int wq = 0;                           // entries per map row: dst_width rounded up to 4
  std::vector<float> map_x, map_y;      // dst_height x dst_width
  std::vector<uint32_t> xy;             // dst_height x wq
  std::vector<uint16_t> frac;
  std::vector<RectWin> win;             // source window per destination tile
  int32_t n_inner = 0, n_edge = 0, n_outside = 0;
  uint32_t* d_xy = nullptr;
  uint16_t* d_frac = nullptr;
  RectWin* d_win = nullptr;
};

static bool side_ok(int v) { return v >= 1 && v <= 4095; }

// initUndistortRectifyMap(K, D, R, P(0:3, 0:3), size, CV_32F), every step in double and in the order the header states
static int build_maps(orbfe_rectifier* r) {
  const orbfe_rectify_camera& c = r->cam;
  double A[9], ir[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += c.P[4 * i + k] * c.R[3 * k + j];
      A[3 * i + j] = s;
    }
  const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
  if (!(det != 0.0) || !isfinite(det)) {
    orbfe_set_error("rectifier: P(0:3, 0:3) x R is singular (determinant %g)", det);
    return ORBFE_ERR_INVALID;
  }
  const double d = 1.0 / det;
  ir[0] = (A[4] * A[8] - A[5] * A[7]) * d;
  ir[1] = (A[2] * A[7] - A[1] * A[8]) * d;
  ir[2] = (A[1] * A[5] - A[2] * A[4]) * d;
  ir[3] = (A[5] * A[6] - A[3] * A[8]) * d;
  ir[4] = (A[0] * A[8] - A[2] * A[6]) * d;
  ir[5] = (A[2] * A[3] - A[0] * A[5]) * d;
  ir[6] = (A[3] * A[7] - A[4] * A[6]) * d;
  ir[7] = (A[1] * A[6] - A[0] * A[7]) * d;
  ir[8] = (A[0] * A[4] - A[1] * A[3]) * d;
  const double fx = c.K[0], fy = c.K[4], u0 = c.K[2], v0 = c.K[5];
  const double k1 = c.D[0], k2 = c.D[1], p1 = c.D[2], p2 = c.D[3], k3 = c.D[4];
  const int w = c.dst_width, h = c.dst_height;
  for (int i = 0; i < h; i++) {
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    float* mx = r->map_x.data() + (size_t)i * w;
    float* my = r->map_y.data() + (size_t)i * w;
    for (int j = 0; j < w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {   // running sums, not j * ir[0]: the result depends on it
      const double ww = 1. / _w, x = _x * ww, y = _y * ww;
      const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
      const double kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
      const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
      const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
      mx[j] = (float)(fx * xd + u0);
      my[j] = (float)(fy * yd + v0);
    }
  }
  return ORBFE_OK;
}

static void rectifier_free(orbfe_rectifier* r) {
  if (!r) return;
  if (r->device >= 0 && (r->d_xy || r->d_frac || r->d_win)) {
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    (void)hipSetDevice(r->device);
    if (r->d_xy) (void)hipFree(r->d_xy);
    if (r->d_frac) (void)hipFree(r->d_frac);
    if (r->d_win) (void)hipFree(r->d_win);
    if (have) (void)hipSetDevice(cur);
  }
  delete r;
}

static int rectifier_build(orbfe_rectifier* r) {
  const orbfe_rectify_camera& c = r->cam;
  const size_t n = (size_t)c.dst_width * c.dst_height;
  r->wq = (c.dst_width + 3) & ~3;
  r->map_x.resize(n);
  r->map_y.resize(n);
  r->xy.assign((size_t)r->wq * c.dst_height, ORBFE_RECT_OUTSIDE << ORBFE_RECT_CLASS_SHIFT);
  r->frac.assign((size_t)r->wq * c.dst_height, 0);
  const int rc = build_maps(r);
  if (rc != ORBFE_OK) return rc;
  for (int i = 0; i < c.dst_height; i++)
    for (int j = 0; j < c.dst_width; j++) {
      const size_t e = (size_t)i * r->wq + j;
      orbfe_rect_entry(r->map_x[(size_t)i * c.dst_width + j], r->map_y[(size_t)i * c.dst_width + j], c.src_width, c.src_height,
                       &r->xy[e], &r->frac[e]);
      const uint32_t cls = r->xy[e] >> ORBFE_RECT_CLASS_SHIFT;
      if (cls == ORBFE_RECT_INNER) r->n_inner++;
      else if (cls == ORBFE_RECT_EDGE) r->n_edge++;
      else r->n_outside++;
    }
  // the source window of every tile without border pixels
  const int tx = (c.dst_width + RECT_TILE_W - 1) / RECT_TILE_W, ty = (c.dst_height + RECT_TILE_H - 1) / RECT_TILE_H;
  r->win.assign((size_t)tx * ty, RectWin{0, 0, 0, 0});
  for (int tj = 0; tj < ty; tj++)
    for (int ti = 0; ti < tx; ti++) {
      int x0 = 4096, x1 = -1, y0 = 4096, y1 = -1;
      bool inner = true;
      for (int i = tj * RECT_TILE_H; inner && i < std::min((tj + 1) * RECT_TILE_H, c.dst_height); i++)
        for (int j = ti * RECT_TILE_W; j < std::min((ti + 1) * RECT_TILE_W, r->wq); j++) {   // the padding entries are OUTSIDE
          const uint32_t e = r->xy[(size_t)i * r->wq + j];
          if (e & ORBFE_RECT_BORDER_MASK) { inner = false; break; }
          const int X = (int)(e & 8191u) - 1, Y = (int)((e >> 13) & 8191u) - 1;
          x0 = std::min(x0, X); x1 = std::max(x1, X + 1); y0 = std::min(y0, Y); y1 = std::max(y1, Y + 1);
        }
      if (!inner) continue;
      x0 &= ~3;
      const int w = (x1 + 1 - x0 + 3) & ~3, h = y1 + 1 - y0;
      if (x0 + w > c.src_width || (w >> 2) * h > RECT_WIN_DWORDS) continue;
      r->win[(size_t)tj * tx + ti] = RectWin{(int16_t)x0, (int16_t)y0, (int16_t)w, (int16_t)h};
    }
  if (r->device < 0) return ORBFE_OK;
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) cur = r->device;
  hipError_t e = hipSetDevice(r->device);
  if (e == hipSuccess) e = hipMalloc((void**)&r->d_xy, r->xy.size() * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&r->d_frac, r->frac.size() * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMemcpy(r->d_xy, r->xy.data(), r->xy.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(r->d_frac, r->frac.data(), r->frac.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&r->d_win, r->win.size() * sizeof(RectWin));
  if (e == hipSuccess) e = hipMemcpy(r->d_win, r->win.data(), r->win.size() * sizeof(RectWin), hipMemcpyHostToDevice);
  (void)hipSetDevice(cur);
  if (e != hipSuccess) {
    orbfe_set_error("rectifier: uploading the map failed: %s", hipGetErrorString(e));
    return ORBFE_ERR_HIP;
  }
  return ORBFE_OK;
}

extern "C" int orbfe_rectifier_create(const orbfe_rectify_camera* cam, int device, orbfe_rectifier** out) {
  if (!cam || !out) return ORBFE_ERR_INVALID;
  *out = nullptr;
  if (!side_ok(cam->src_width) || !side_ok(cam->src_height) || !side_ok(cam->dst_width) || !side_ok(cam->dst_height)) {
    orbfe_set_error("rectifier: source %d x %d, destination %d x %d: 1 .. 4095 per side", cam->src_width, cam->src_height,
                    cam->dst_width, cam->dst_height);
    return ORBFE_ERR_INVALID;
  }
  if (cam->K[1] != 0.0) {
    orbfe_set_error("rectifier: a camera matrix with skew (K[0][1] = %g) is not supported", cam->K[1]);
    return ORBFE_ERR_INVALID;
  }
  if (device < -1) {
    orbfe_set_error("rectifier: device %d (-1: host-only handle, else a device index)", device);
    return ORBFE_ERR_INVALID;
  }
  if (device >= 0) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
      orbfe_set_error("no HIP device available (create the rectifier with device -1 for the host routines alone)");
      return ORBFE_ERR_NO_DEVICE;
    }
    if (device >= ndev) {
      orbfe_set_error("rectifier: device %d of %d", device, ndev);
      return ORBFE_ERR_INVALID;
    }
  }
  orbfe_rectifier* r = new (std::nothrow) orbfe_rectifier();
  if (!r) return ORBFE_ERR_ALLOC;
  r->cam = *cam;
  r->device = device;
  int rc;
  try {
    rc = rectifier_build(r);
  } catch (...) {
    orbfe_set_error("orbfe_rectifier_create: out of host memory");
    rc = ORBFE_ERR_ALLOC;
  }
  if (rc != ORBFE_OK) {
    rectifier_free(r);
    return rc;
  }
  *out = r;
  return ORBFE_OK;
}

extern "C" int orbfe_rectifier_destroy(orbfe_rectifier* r) {
  rectifier_free(r);
  return ORBFE_OK;
}

extern "C" int orbfe_rectifier_info(const orbfe_rectifier* r, orbfe_rectify_camera* cam, int* device) {
  if (!r) return ORBFE_ERR_INVALID;
  if (cam) *cam = r->cam;
  if (device) *device = r->device;
  return ORBFE_OK;
}

extern "C" int orbfe_rectifier_maps(const orbfe_rectifier* r, float* map_x, float* map_y) {
  if (!r || !map_x || !map_y) return ORBFE_ERR_INVALID;
  std::copy(r->map_x.begin(), r->map_x.end(), map_x);
  std::copy(r->map_y.begin(), r->map_y.end(), map_y);
  return ORBFE_OK;
}

extern "C" int orbfe_rectifier_coverage(const orbfe_rectifier* r, int32_t* inner, int32_t* edge, int32_t* outside) {
  if (!r) return ORBFE_ERR_INVALID;
  if (inner) *inner = r->n_inner;
  if (edge) *edge = r->n_edge;
  if (outside) *outside = r->n_outside;
  return ORBFE_OK;
}

extern "C" int orbfe_rectify_image(const orbfe_rectifier* r, const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride) {
  if (!r || !src || !dst) return ORBFE_ERR_INVALID;
  const orbfe_rectify_camera& c = r->cam;
  if (src_stride < c.src_width || dst_stride < c.dst_width) {
    orbfe_set_error("rectify image: strides %d / %d below the widths %d / %d", src_stride, dst_stride, c.src_width, c.dst_width);
    return ORBFE_ERR_INVALID;
  }
  for (int i = 0; i < c.dst_height; i++) {
    const uint32_t* xy = r->xy.data() + (size_t)i * r->wq;
    const uint16_t* fr = r->frac.data() + (size_t)i * r->wq;
    uint8_t* d = dst + (size_t)i * dst_stride;
    for (int j = 0; j < c.dst_width; j++) d[j] = orbfe_rect_pixel(src, (size_t)src_stride, c.src_width, c.src_height, xy[j], fr[j]);
  }
  return ORBFE_OK;
}

extern "C" int orbfe_rectify_batch_device(orbfe_rectifier* r, const uint8_t* d_src, int n_images, int src_pitch, size_t src_image_bytes,
                                          uint8_t* d_dst, int dst_pitch, size_t dst_image_bytes, void* stream) {
  if (!r || n_images < 0) {
    orbfe_set_error("rectify batch: a rectifier and n_images >= 0 are required");
    return ORBFE_ERR_INVALID;
  }
  if (r->device < 0) {
    orbfe_set_error("rectify batch: a host-only rectifier (created with device -1) has no map on a device; liborbfe has no CPU fallback");
    return ORBFE_ERR_NO_DEVICE;
  }
  const orbfe_rectify_camera& c = r->cam;
  if (src_pitch < c.src_width || dst_pitch < c.dst_width) {
    orbfe_set_error("rectify batch: pitches %d / %d below the widths %d / %d", src_pitch, dst_pitch, c.src_width, c.dst_width);
    return ORBFE_ERR_INVALID;
  }
  const size_t src_span = (size_t)(c.src_height - 1) * (size_t)src_pitch + (size_t)c.src_width;
  const size_t dst_span = (size_t)(c.dst_height - 1) * (size_t)dst_pitch + (size_t)c.dst_width;
  if (src_image_bytes < src_span || dst_image_bytes < dst_span) {
    orbfe_set_error("rectify batch: image strides %zu / %zu too small for %d rows of pitch %d / %d rows of pitch %d", src_image_bytes,
                    dst_image_bytes, c.src_height, src_pitch, c.dst_height, dst_pitch);
    return ORBFE_ERR_INVALID;
  }
  if (n_images == 0) return ORBFE_OK;
  if (!d_src || !d_dst) {
    orbfe_set_error("rectify batch: source and destination are required");
    return ORBFE_ERR_INVALID;
  }
  const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (size_t)(n_images - 1) * src_image_bytes + src_span;
  const uintptr_t d0 = (uintptr_t)d_dst, d1 = d0 + (size_t)(n_images - 1) * dst_image_bytes + dst_span;
  if (s0 < d1 && d0 < s1) {
    orbfe_set_error("rectify batch: source and destination overlap (a pixel reads rows other pixels write)");
    return ORBFE_ERR_INVALID;
  }
  RectMap m;
  m.xy = r->d_xy;
  m.frac = r->d_frac;
  m.win = r->d_win;
  m.wq = r->wq;
  m.dst_w = c.dst_width;
  m.dst_h = c.dst_height;
  m.src_w = c.src_width;
  m.src_h = c.src_height;
  orbfe_launch_rectify(m, d_src, n_images, src_pitch, src_image_bytes, d_dst, dst_pitch, dst_image_bytes, (hipStream_t)stream);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    orbfe_set_error("kernel launch failed: %s", hipGetErrorString(le));
    return ORBFE_ERR_HIP;
  }
  return ORBFE_OK;
}
