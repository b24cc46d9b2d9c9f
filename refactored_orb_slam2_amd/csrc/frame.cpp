// frame.cpp -- C ABI of the per-keypoint tail of Frame::Frame: lens undistortion, image bounds, RGB-D depth (include/orbfe.h).
// The two host helpers run frame_internal.h's arithmetic on the CPU for calibration-time use (four corners, a few points); the batch
// entry point validates and launches frame_kernels.hip.  No CPU fallback: without a device the batch entry point is an error.
#include <math.h>

#include "frame_internal.h"

void orbfe_set_error(const char* fmt, ...);

static bool cal_ok(const orbfe_calibration* cal) {
  if (!cal) return false;
  if (cal->fx == 0.0f || cal->fy == 0.0f) {
    orbfe_set_error("calibration: fx and fy must be non-zero (fx %g, fy %g)", (double)cal->fx, (double)cal->fy);
    return false;
  }
  return true;
}

extern "C" int orbfe_undistort_points(const orbfe_calibration* cal, const float* xy, int n, float* xy_un) {
  if (!cal_ok(cal) || n < 0 || (n > 0 && (!xy || !xy_un))) return ORBFE_ERR_INVALID;
  const FrameCam k = orbfe_frame_cam(*cal, ORBFE_DEPTH_NONE);
  for (int i = 0; i < n; i++) {
    float x, y;
    orbfe_key_un(k, xy[2 * i], xy[2 * i + 1], &x, &y);
    xy_un[2 * i] = x;
    xy_un[2 * i + 1] = y;
  }
  return ORBFE_OK;
}

extern "C" int orbfe_image_bounds(const orbfe_calibration* cal, int width, int height, float* min_x, float* max_x, float* min_y,
                                  float* max_y) {
  if (!cal_ok(cal) || !min_x || !max_x || !min_y || !max_y) return ORBFE_ERR_INVALID;
  if (width < 1 || height < 1 || width > 4095 || height > 4095) {
    orbfe_set_error("image size %d x %d: 1 .. 4095 per side", width, height);
    return ORBFE_ERR_INVALID;
  }
  const FrameCam k = orbfe_frame_cam(*cal, ORBFE_DEPTH_NONE);
  if (!k.undistort) {   // Frame.cc:469-474
    *min_x = 0.0f;
    *max_x = (float)width;
    *min_y = 0.0f;
    *max_y = (float)height;
    return ORBFE_OK;
  }
  const float cx[4] = {0.0f, (float)width, 0.0f, (float)width}, cy[4] = {0.0f, 0.0f, (float)height, (float)height};
  float ux[4], uy[4];
  for (int c = 0; c < 4; c++) orbfe_undistort_point(k, cx[c], cy[c], &ux[c], &uy[c]);
  // std::min / std::max of Frame.cc:464-467: min(a, b) = (b < a) ? b : a, max(a, b) = (a < b) ? b : a
  *min_x = ux[2] < ux[0] ? ux[2] : ux[0];
  *max_x = ux[1] < ux[3] ? ux[3] : ux[1];
  *min_y = uy[1] < uy[0] ? uy[1] : uy[0];
  *max_y = uy[2] < uy[3] ? uy[3] : uy[2];
  return ORBFE_OK;
}

extern "C" int orbfe_undistort_frames_device(int n_frames, const orbfe_keypoint* d_kps, const int32_t* d_n, int cap,
                                             const orbfe_calibration* cal, int depth_format, const void* d_depth, int width, int height,
                                             int depth_pitch, size_t depth_image_bytes, orbfe_keypoint* d_kps_un, float* d_u_right,
                                             float* d_depth_out, int32_t* d_n_depth, void* stream) {
  if (!d_kps || !d_n || !d_kps_un || n_frames < 0 || cap < 1) {
    orbfe_set_error("undistort frames: keypoints, counts and output keypoints are required; n_frames >= 0, cap >= 1");
    return ORBFE_ERR_INVALID;
  }
  if (!cal_ok(cal)) return ORBFE_ERR_INVALID;
  if (depth_format != ORBFE_DEPTH_NONE && depth_format != ORBFE_DEPTH_U16 && depth_format != ORBFE_DEPTH_F32) {
    orbfe_set_error("undistort frames: unknown depth format %d", depth_format);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_kps & 3) || ((uintptr_t)d_kps_un & 3) || ((uintptr_t)d_n & 3) || ((uintptr_t)d_u_right & 3) ||
      ((uintptr_t)d_depth_out & 3) || ((uintptr_t)d_n_depth & 3)) {
    orbfe_set_error("undistort frames: records and outputs must be 4-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  if (depth_format != ORBFE_DEPTH_NONE) {
    const size_t elem = depth_format == ORBFE_DEPTH_U16 ? 2 : 4;
    if (!d_depth || !d_u_right || !d_depth_out || !d_n_depth) {
      orbfe_set_error("undistort frames: a depth format needs the map, u_right, depth and n_depth");
      return ORBFE_ERR_INVALID;
    }
    if (width < 1 || height < 1 || width > 4095 || height > 4095) {
      orbfe_set_error("depth map of %d x %d: 1 .. 4095 per side", width, height);
      return ORBFE_ERR_INVALID;
    }
    if (depth_pitch < 0 || (size_t)depth_pitch < (size_t)width * elem ||
        depth_image_bytes < (size_t)(height - 1) * (size_t)depth_pitch + (size_t)width * elem) {
      orbfe_set_error("depth map: pitch %d / image stride %zu too small for %d x %d samples of %zu bytes", depth_pitch, depth_image_bytes,
                      width, height, elem);
      return ORBFE_ERR_INVALID;
    }
    if (((uintptr_t)d_depth % elem) || ((size_t)depth_pitch % elem) || (depth_image_bytes % elem)) {
      orbfe_set_error("depth map: pointer, pitch and image stride must be multiples of the %zu-byte sample", elem);
      return ORBFE_ERR_INVALID;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    orbfe_set_error("no HIP device available (liborbfe has no CPU fallback)");
    return ORBFE_ERR_NO_DEVICE;
  }
  if (n_frames == 0) return ORBFE_OK;
  const FrameCam k = orbfe_frame_cam(*cal, depth_format);
  orbfe_launch_undistort_frames(n_frames, d_kps, d_n, cap, k, depth_format, (const uint8_t*)d_depth, width, height, depth_pitch,
                                depth_image_bytes, d_kps_un, d_u_right, d_depth_out, d_n_depth, (hipStream_t)stream);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    orbfe_set_error("kernel launch failed: %s", hipGetErrorString(le));
    return ORBFE_ERR_HIP;
  }
  return ORBFE_OK;
}
