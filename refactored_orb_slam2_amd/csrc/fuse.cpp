// fuse.cpp -- host side of the resident fuse batch: K target keyframes in HBM with their grids built once and one persistent table of
// candidate map points, searched row by row (point i in target k) in one launch (fuse_kernels.hip).  No CPU fallback.
//
// Reference behaviour (L/ = Source/Libraries/ORB_SLAM2/):
//   LocalMapping::SearchInNeighbors            L/src/LocalMapping.cc:425-509
//   ORBmatcher::Fuse / Fuse with Sim3          L/src/ORBmatcher.cc:766-907, 909-1027
//   MapPoint::Replace                          L/src/MapPoint.cc:172-206
#include <string.h>

#include <mutex>

#include "fuse_internal.h"
#include "host_internal.h"

// What a handle allocates: a stream, device blocks and pinned mirrors that only grow.  A batch lives for one keyframe, and allocating
// and freeing these costs about 1 ms, several searches' worth (profiles/search_in_neighbors.md), so a destroyed handle leaves them to
// the calling thread's next handle; orbfe_thread_release() frees them (a thread that ends without it keeps them, as it keeps its matcher
// handle).
struct FuseMem {
  int device = 0;
  hipStream_t stream = nullptr;
  void* d_targets = nullptr;        // host form: the one packed block [n | cams | 1/sigma2 | keys | desc | u_right]
  void* h_targets = nullptr;        //   and its pinned mirror
  size_t b_targets = 0;
  void* d_grid = nullptr;           // [cell_start | cell_idx | cell_rec] of the K targets
  size_t b_grid = 0;
  orbfe_kf_point* d_table = nullptr;   // the resident point table
  int table_cap = 0;
  // staging of the host search: [records | index list | mask | results], device block and pinned mirror
  uint8_t *d_stage = nullptr, *h_stage = nullptr;
  size_t stage_bytes = 0;
};
struct orbfe_fuse_batch : FuseMem {
  int K = 0, cap = 1, mode = 0;
  bool borrowed = false;            // create_device: the target arrays are the caller's
  FrameBatch fb{};                  // keys / desc / u_right / n and the grids
  const orbfe_kf_camera* d_cams = nullptr;
  const float* d_inv = nullptr;
  const float* d_geo = nullptr;     // [K][4] min_x, min_y, gw_inv, gh_inv where the targets' image bounds differ, else nullptr
  std::vector<float> geo;           //   and its host copy: such targets get a grid-build launch each
  int n_points = 0;
  // the caller's streams this handle has enqueued work on, each with an event recorded behind the last of it: what destroy and a
  // growing table wait for besides the handle's own stream (the rest of the device -- another thread's extraction -- is not theirs to wait for)
  std::vector<std::pair<hipStream_t, hipEvent_t>> foreign;
  std::mutex mu;
};

static int note_foreign(orbfe_fuse_batch* b, hipStream_t s) {
  if (s == b->stream) return ORBFE_OK;
  hipEvent_t ev = nullptr;
  for (auto& f : b->foreign)
    if (f.first == s) ev = f.second;
  if (!ev) {
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    b->foreign.push_back(std::make_pair(s, ev));
  }
  HIPCHK(hipEventRecord(ev, s));
  return ORBFE_OK;
}
static void wait_foreign(orbfe_fuse_batch* b, bool forget) {
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  for (auto& f : b->foreign) {
    (void)hipEventSynchronize(f.second);
    if (forget) (void)hipEventDestroy(f.second);
  }
  if (forget) b->foreign.clear();
}
struct FuseSpare {
  FuseMem m;
  bool full = false;
};
static thread_local FuseSpare t_spare;

static void free_mem(FuseMem& m) {
  (void)hipSetDevice(m.device);
  void* dev[] = {m.d_targets, m.d_grid, m.d_table, m.d_stage};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  if (m.h_targets) (void)hipHostFree(m.h_targets);
  if (m.h_stage) (void)hipHostFree(m.h_stage);
  if (m.stream) (void)hipStreamDestroy(m.stream);
  m = FuseMem();
}
void orbfe_fuse_release_spare() {
  if (t_spare.full) free_mem(t_spare.m);
  t_spare.full = false;
}

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

static bool mode_ok(int mode) { return mode == ORBFE_KF_FUSE || mode == ORBFE_KF_FUSE_SIM3; }

// a device block of at least `bytes` (and, with `h`, its pinned mirror); `have` is what the pair holds now
static int grow(void** d, void** h, size_t& have, size_t bytes) {
  if (*d && bytes <= have) return ORBFE_OK;
  if (*d) HIPCHK(hipFree(*d));
  *d = nullptr;
  if (h && *h) HIPCHK(hipHostFree(*h));
  if (h) *h = nullptr;
  have = 0;
  bytes = (bytes + 65535) & ~(size_t)65535;
  HIPCHK(hipMalloc(d, bytes));
  if (h) HIPCHK(hipHostMalloc(h, bytes, hipHostMallocDefault));
  have = bytes;
  return ORBFE_OK;
}

// the grids of the K targets and the stream: what both create forms end with (fb.keys / desc / u_right / n / cap and the bounds are set)
static int finish_create(orbfe_fuse_batch* b, hipStream_t build_stream) {
  const size_t F = (size_t)std::max(b->K, 1);
  const size_t b_cs = up256(F * (GRID_CELLS + 1) * sizeof(int32_t)), b_ci = up256(F * b->cap * sizeof(int32_t)), b_cr = F * b->cap * 16;
  int rc;
  if ((rc = grow(&b->d_grid, nullptr, b->b_grid, b_cs + b_ci + b_cr))) return rc;
  b->fb.cell_start = (int32_t*)b->d_grid;
  b->fb.cell_idx = (int32_t*)((uint8_t*)b->d_grid + b_cs);
  b->fb.cell_rec = (uint32_t*)((uint8_t*)b->d_grid + b_cs + b_ci);
  if (b->K > 0 && b->geo.empty()) {
    orbfe_launch_grid_build(b->fb, b->K, build_stream);   // one set of bounds: ONE launch for all K
    HIPCHK(hipGetLastError());
  }
  for (int k = 0; k < b->K && !b->geo.empty(); k++) {     // bounds of their own: the grid geometry is a launch constant, a launch per target
    FrameBatch f = b->fb;
    const size_t o = (size_t)k * b->cap;
    f.keys += o; f.desc += o * 32; f.n += k;
    if (f.u_right) f.u_right += o;
    f.cell_start += (size_t)k * (GRID_CELLS + 1); f.cell_idx += o; f.cell_rec += o * 4;
    f.min_x = b->geo[4 * k]; f.min_y = b->geo[4 * k + 1]; f.gw_inv = b->geo[4 * k + 2]; f.gh_inv = b->geo[4 * k + 3];
    orbfe_launch_grid_build(f, 1, build_stream);
    HIPCHK(hipGetLastError());
  }
  return ORBFE_OK;
}

static int new_handle(orbfe_fuse_batch** out, int K, int cap, int mode, float min_x, float max_x, float min_y, float max_y) {
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) device = 0;
  HIPCHK(hipSetDevice(device));
  orbfe_fuse_batch* b = new orbfe_fuse_batch();
  b->device = device; b->K = K; b->cap = cap; b->mode = mode;
  b->fb.cap = cap;
  b->fb.min_x = min_x;
  b->fb.min_y = min_y;
  b->fb.gw_inv = (float)ORBFE_GRID_COLS / (max_x - min_x);   // mfGridElementWidthInv / HeightInv, L/src/Frame.cc:109-112
  b->fb.gh_inv = (float)ORBFE_GRID_ROWS / (max_y - min_y);
  if (t_spare.full && t_spare.m.device == device) {   // what this thread's last handle left
    static_cast<FuseMem&>(*b) = t_spare.m;
    t_spare = FuseSpare();
  } else {
    const hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete b;
      return hip_status("hipStreamCreate", e);
    }
  }
  *out = b;
  return ORBFE_OK;
}

extern "C" int orbfe_fuse_batch_destroy(orbfe_fuse_batch* b) {
  if (!b) return ORBFE_OK;
  (void)hipSetDevice(b->device);
  wait_foreign(b, true);   // its own stream and every caller's stream it was used with: nothing still reads the blocks the next handle takes
  if (!t_spare.full && b->stream) {
    t_spare.m = static_cast<FuseMem&>(*b);
    t_spare.full = true;
  } else {
    free_mem(*b);
  }
  delete b;
  return ORBFE_OK;
}

// What orbfe_fuse_batch_create refuses, before a device is looked for.  *cap_out = the largest target (at least 1).
int orbfe_fuse_validate_targets(int K, const orbfe_frame_view* targets, const orbfe_kf_camera* cams, const float* inv_level_sigma2, int mode,
                                int* cap_out) {
  if (K < 0 || !mode_ok(mode) || (K > 0 && (!targets || !cams)) || (K > 0 && mode == ORBFE_KF_FUSE && !inv_level_sigma2)) {
    orbfe_set_error("fuse batch: K >= 0, mode ORBFE_KF_FUSE or ORBFE_KF_FUSE_SIM3, no null array (1 / sigma2 tables: ORBFE_KF_FUSE)");
    return ORBFE_ERR_INVALID;
  }
  int cap = 1;
  for (int k = 0; k < K; k++) {
    const orbfe_frame_view& f = targets[k];
    if (f.n < 0 || f.n > 65535 || (f.n > 0 && (!f.keys_un || !f.desc)) || !(f.max_x > f.min_x) || !(f.max_y > f.min_y)) {
      orbfe_set_error("fuse batch: target %d of %d keypoints: 0 .. 65535, with keypoints, descriptors and non-empty bounds", k, f.n);
      return ORBFE_ERR_INVALID;
    }
    if (cams[k].n_levels < 1 || cams[k].n_levels > ORBFE_MAX_LEVELS) {
      orbfe_set_error("fuse batch: target %d has n_levels = %d: 1 .. %d", k, cams[k].n_levels, ORBFE_MAX_LEVELS);
      return ORBFE_ERR_INVALID;
    }
    cap = std::max(cap, f.n);
  }
  *cap_out = cap;
  return ORBFE_OK;
}

extern "C" int orbfe_fuse_batch_create(int K, const orbfe_frame_view* targets, const orbfe_kf_camera* cams, const float* inv_level_sigma2,
                                       int mode, orbfe_fuse_batch** out) {
  if (!out) return ORBFE_ERR_INVALID;
  *out = nullptr;
  int cap = 1, rc;
  if ((rc = orbfe_fuse_validate_targets(K, targets, cams, inv_level_sigma2, mode, &cap))) return rc;
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  orbfe_fuse_batch* b = nullptr;
  const bool any = K > 0;
  if ((rc = new_handle(&b, K, cap, mode, any ? targets[0].min_x : 0.f, any ? targets[0].max_x : 1.f, any ? targets[0].min_y : 0.f,
                       any ? targets[0].max_y : 1.f)))
    return rc;
  // one packed block [n | cameras | 1 / sigma2 | keypoints | descriptors | mvuRight], target k at offset k * cap of the last three
  const size_t F = (size_t)std::max(K, 1), rows = F * cap;
  Layout L;
  const size_t o_n = L.add(F * sizeof(int32_t)), o_cam = L.add(F * sizeof(orbfe_kf_camera)), o_inv = L.add(F * ORBFE_MAX_LEVELS * sizeof(float)),
               o_keys = L.add(rows * sizeof(orbfe_keypoint)), o_desc = L.add(rows * 32), o_ur = L.add(rows * sizeof(float)),
               o_geo = L.add(F * 4 * sizeof(float));
  if ((rc = grow(&b->d_targets, &b->h_targets, b->b_targets, L.off))) {
    orbfe_fuse_batch_destroy(b);
    return rc;
  }
  uint8_t* hp = (uint8_t*)b->h_targets;
  memset(hp + o_inv, 0, F * ORBFE_MAX_LEVELS * sizeof(float));   // (rows behind a target's n keypoints are never read: no other fill)
  bool any_ur = false, own_bounds = false;
  for (int k = 0; k < K; k++) {
    const orbfe_frame_view &f = targets[k], &f0 = targets[0];
    any_ur = any_ur || (f.n > 0 && f.u_right);
    own_bounds = own_bounds || f.min_x != f0.min_x || f.max_x != f0.max_x || f.min_y != f0.min_y || f.max_y != f0.max_y;
    float* g = (float*)(hp + o_geo) + 4 * k;   // mfGridElementWidthInv / HeightInv of the target's own bounds
    g[0] = f.min_x; g[1] = f.min_y; g[2] = (float)ORBFE_GRID_COLS / (f.max_x - f.min_x); g[3] = (float)ORBFE_GRID_ROWS / (f.max_y - f.min_y);
  }
  if (own_bounds) b->geo.assign((const float*)(hp + o_geo), (const float*)(hp + o_geo) + 4 * (size_t)K);
  for (int k = 0; k < K; k++) {
    const orbfe_frame_view& f = targets[k];
    ((int32_t*)(hp + o_n))[k] = f.n;
    ((orbfe_kf_camera*)(hp + o_cam))[k] = cams[k];
    if (inv_level_sigma2)   // the first n_levels floats, zero behind them: what orbfe_kf_search stages
      memcpy((float*)(hp + o_inv) + (size_t)k * ORBFE_MAX_LEVELS, inv_level_sigma2 + (size_t)k * ORBFE_MAX_LEVELS, sizeof(float) * cams[k].n_levels);
    float* ur = (float*)(hp + o_ur) + (size_t)k * cap;
    for (int i = 0; i < cap; i++) ur[i] = -1.0f;   // a target without mvuRight: the grid record's value for "no right coordinate"
    if (f.n == 0) continue;
    memcpy((orbfe_keypoint*)(hp + o_keys) + (size_t)k * cap, f.keys_un, sizeof(orbfe_keypoint) * (size_t)f.n);
    memcpy(hp + o_desc + (size_t)k * cap * 32, f.desc, (size_t)32 * f.n);
    if (f.u_right) memcpy(ur, f.u_right, sizeof(float) * (size_t)f.n);
  }
  uint8_t* dp = (uint8_t*)b->d_targets;
  const hipError_t e = hipMemcpyAsync(dp, hp, L.off, hipMemcpyHostToDevice, b->stream);
  b->fb.n = (const int32_t*)(dp + o_n);
  b->fb.keys = (const orbfe_keypoint*)(dp + o_keys);
  b->fb.desc = dp + o_desc;
  b->fb.u_right = any_ur ? (const float*)(dp + o_ur) : nullptr;
  b->d_cams = (const orbfe_kf_camera*)(dp + o_cam);
  b->d_inv = inv_level_sigma2 ? (const float*)(dp + o_inv) : nullptr;
  b->d_geo = own_bounds ? (const float*)(dp + o_geo) : nullptr;
  rc = e != hipSuccess ? hip_status("orbfe_fuse_batch_create", e) : finish_create(b, b->stream);
  const hipError_t e2 = hipStreamSynchronize(b->stream);   // also on an error: the copy may still read the pinned block
  if (!rc) rc = hip_status("orbfe_fuse_batch_create", e2);
  if (rc) {
    orbfe_fuse_batch_destroy(b);
    return rc;
  }
  *out = b;
  return ORBFE_OK;
}

extern "C" int orbfe_fuse_batch_create_device(int K, const orbfe_keypoint* d_keys, const uint8_t* d_desc, const float* d_u_right,
                                              const int32_t* d_n, int cap, float min_x, float max_x, float min_y, float max_y,
                                              const orbfe_kf_camera* d_cams, const float* d_inv_level_sigma2, int mode, void* stream,
                                              orbfe_fuse_batch** out) {
  if (!out) return ORBFE_ERR_INVALID;
  *out = nullptr;
  if (K < 0 || !mode_ok(mode) || cap < 1 || cap > 65535 || !(max_x > min_x) || !(max_y > min_y) ||
      (K > 0 && (!d_keys || !d_desc || !d_n || !d_cams)) || (K > 0 && mode == ORBFE_KF_FUSE && !d_inv_level_sigma2)) {
    orbfe_set_error("fuse batch: K >= 0, cap 1 .. 65535, non-empty bounds, mode ORBFE_KF_FUSE or ORBFE_KF_FUSE_SIM3, no null array");
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_desc & 15) || ((uintptr_t)d_keys & 3)) {
    orbfe_set_error("descriptors must be 16-byte aligned, keypoints 4-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  orbfe_fuse_batch* b = nullptr;
  int rc;
  if ((rc = new_handle(&b, K, cap, mode, min_x, max_x, min_y, max_y))) return rc;
  b->borrowed = true;
  b->fb.keys = d_keys; b->fb.desc = d_desc; b->fb.u_right = d_u_right; b->fb.n = d_n;
  b->d_cams = d_cams;
  b->d_inv = d_inv_level_sigma2;
  if ((rc = finish_create(b, stream ? (hipStream_t)stream : b->stream)) || (stream && (rc = note_foreign(b, (hipStream_t)stream)))) {
    orbfe_fuse_batch_destroy(b);
    return rc;
  }
  *out = b;
  return ORBFE_OK;
}

// K x n_points rows within int32_t (row indices and the launch grid are ints)
int orbfe_fuse_validate_rows(int K, int n_points) {
  if ((int64_t)K * (int64_t)n_points > (int64_t)INT32_MAX) {
    orbfe_set_error("fuse search: K x n_points = %d x %d rows: at most 2 147 483 647", K, n_points);
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
}

// What both search forms refuse of their scalar arguments.
static int validate_search(const orbfe_fuse_batch* b, const void* points, int n_points, const void* point_idx, int n_idx, int first_target,
                           const void* results) {
  if (!b) return ORBFE_ERR_INVALID;
  const bool partial = point_idx != nullptr;
  if (n_points < 0 || first_target < 0 || first_target > b->K || (partial && n_idx < 0)) {
    orbfe_set_error("fuse search: n_points >= 0, n_idx >= 0, first_target 0 .. K (%d)", b->K);
    return ORBFE_ERR_INVALID;
  }
  if (orbfe_fuse_validate_rows(b->K, n_points)) return ORBFE_ERR_INVALID;
  if (partial && n_points != b->n_points) {
    orbfe_set_error("fuse search: a partial search states the resident table's size (%d), not %d", b->n_points, n_points);
    return ORBFE_ERR_INVALID;
  }
  const int n_rec = partial ? n_idx : n_points;
  if ((n_rec > 0 && !points) || (n_rec > 0 && b->K > first_target && !results)) {
    orbfe_set_error("fuse search: null records or results");
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
}

// The launches of one search on `s`: the records into the resident table, then every selected row.  Rows go to `out` as FuseRows says.
static int search_enqueue(orbfe_fuse_batch* b, const orbfe_kf_point* d_points, int n_points, const int32_t* d_idx, int n_idx, int first_target,
                          const uint8_t* d_skip, orbfe_kf_result* out, int out_first, int out_stride, int out_by_list, hipStream_t s) {
  const bool partial = d_idx != nullptr;
  if (!partial) {
    if (n_points > b->table_cap) {
      wait_foreign(b, false);   // nothing of an earlier search, on whichever stream it ran, still reads the old table
      if (b->d_table) HIPCHK(hipFree(b->d_table));
      b->d_table = nullptr;
      b->table_cap = 0;
      HIPCHK(hipMalloc((void**)&b->d_table, sizeof(orbfe_kf_point) * (size_t)n_points));
      b->table_cap = n_points;
    }
    b->n_points = n_points;
    if (n_points > 0) HIPCHK(hipMemcpyAsync(b->d_table, d_points, sizeof(orbfe_kf_point) * (size_t)n_points, hipMemcpyDeviceToDevice, s));
  } else {
    orbfe_launch_fuse_scatter(b->d_table, b->n_points, d_points, d_idx, n_idx, s);
  }
  FuseRows a;
  a.F = b->fb;
  a.cams = b->d_cams;
  a.inv_sigma2 = b->d_inv;
  a.geo = b->d_geo;
  a.points = b->d_table;
  a.point_idx = d_idx;
  a.skip = d_skip;
  a.out = out; a.out_first = out_first; a.out_stride = out_stride; a.out_by_list = out_by_list;
  a.n_points = b->n_points;
  a.n_rows = partial ? n_idx : n_points;
  a.first_target = first_target;
  a.n_targets = b->K;
  a.mode = b->mode;
  orbfe_launch_fuse_rows(a, s);
  return hip_status("kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_fuse_batch_search_device(orbfe_fuse_batch* b, const orbfe_kf_point* d_points, int n_points, const int32_t* d_point_idx,
                                              int n_idx, int first_target, const uint8_t* d_skip, orbfe_kf_result* d_results, void* stream) {
  if (!b) return ORBFE_ERR_INVALID;
  std::lock_guard<std::mutex> lk(b->mu);   // before the validation: it reads the resident table's size, which a search writes
  int rc;
  if ((rc = validate_search(b, d_points, n_points, d_point_idx, n_idx, first_target, d_results))) return rc;
  HIPCHK(hipSetDevice(b->device));
  const hipStream_t s = stream ? (hipStream_t)stream : b->stream;
  if ((rc = search_enqueue(b, d_points, n_points, d_point_idx, n_idx, first_target, d_skip, d_results, 0, n_points, 0, s))) return rc;
  return note_foreign(b, s);
}

// Sizes of the host search's staging block: [records | index list | mask | results]; the results are the searched rows only, target
// after target (a partial search: n_idx rows per target, in list order).
FuseStage orbfe_fuse_stage_layout(int K, int n_points, int n_rec, bool partial, bool with_skip, int first_target) {
  Layout L;
  FuseStage st;
  st.o_pts = L.add(sizeof(orbfe_kf_point) * (size_t)n_rec);
  st.o_idx = L.add(partial ? sizeof(int32_t) * (size_t)n_rec : 0);
  st.o_skip = L.add(with_skip ? (size_t)K * (size_t)n_points : 0);
  st.o_res = L.add(sizeof(orbfe_kf_result) * (size_t)(K - first_target) * (size_t)n_rec);
  st.total = L.off;
  return st;
}

// point_idx strictly ascending and within [0, n_points)
int orbfe_fuse_validate_index(const int32_t* point_idx, int n_idx, int n_points) {
  for (int j = 0; j < n_idx; j++)
    if (point_idx[j] < 0 || point_idx[j] >= n_points || (j > 0 && point_idx[j] <= point_idx[j - 1])) {
      orbfe_set_error("fuse search: point_idx[%d] = %d: strictly ascending, 0 .. %d", j, point_idx[j], n_points - 1);
      return ORBFE_ERR_INVALID;
    }
  return ORBFE_OK;
}

// Scatter of the staged result rows into the caller's K x n_points array: only the searched rows are written.
void orbfe_fuse_unstage_results(const orbfe_kf_result* staged, int K, int n_points, const int32_t* point_idx, int n_rec, int first_target,
                                orbfe_kf_result* results) {
  for (int k = first_target; k < K; k++) {
    const orbfe_kf_result* src = staged + (size_t)(k - first_target) * n_rec;
    orbfe_kf_result* dst = results + (size_t)k * n_points;
    if (!point_idx) memcpy(dst, src, sizeof(orbfe_kf_result) * (size_t)n_rec);
    else
      for (int j = 0; j < n_rec; j++) dst[point_idx[j]] = src[j];
  }
}

extern "C" int orbfe_fuse_batch_search(orbfe_fuse_batch* b, const orbfe_kf_point* points, int n_points, const int32_t* point_idx, int n_idx,
                                       int first_target, const uint8_t* skip, orbfe_kf_result* results) {
  if (!b) return ORBFE_ERR_INVALID;
  std::lock_guard<std::mutex> lk(b->mu);   // before the validation: it reads the resident table's size, which a search writes
  int rc;
  if ((rc = validate_search(b, points, n_points, point_idx, n_idx, first_target, results))) return rc;
  const bool partial = point_idx != nullptr;
  const int n_rec = partial ? n_idx : n_points;
  if (partial && (rc = orbfe_fuse_validate_index(point_idx, n_idx, n_points))) return rc;
  HIPCHK(hipSetDevice(b->device));
  if (!partial && n_points == 0) {   // an empty table: nothing to launch
    b->n_points = 0;
    return ORBFE_OK;
  }
  if (n_rec == 0) return ORBFE_OK;
  const FuseStage st = orbfe_fuse_stage_layout(b->K, n_points, n_rec, partial, skip != nullptr, first_target);
  if (st.total > b->stage_bytes) {
    if (b->d_stage) HIPCHK(hipFree(b->d_stage));
    b->d_stage = nullptr;
    if (b->h_stage) HIPCHK(hipHostFree(b->h_stage));
    b->h_stage = nullptr;
    b->stage_bytes = 0;
    const size_t bytes = (st.total + 65535) & ~(size_t)65535;
    HIPCHK(hipMalloc((void**)&b->d_stage, bytes));
    HIPCHK(hipHostMalloc((void**)&b->h_stage, bytes, hipHostMallocDefault));
    b->stage_bytes = bytes;
  }
  memcpy(b->h_stage + st.o_pts, points, sizeof(orbfe_kf_point) * (size_t)n_rec);
  if (partial) memcpy(b->h_stage + st.o_idx, point_idx, sizeof(int32_t) * (size_t)n_rec);
  if (skip) memcpy(b->h_stage + st.o_skip, skip, (size_t)b->K * (size_t)n_points);
  hipError_t e = hipMemcpyAsync(b->d_stage, b->h_stage, st.o_res, hipMemcpyHostToDevice, b->stream);   // one packed upload
  rc = hip_status("orbfe_fuse_batch_search", e);
  const size_t b_res = sizeof(orbfe_kf_result) * (size_t)(b->K - first_target) * (size_t)n_rec;
  if (!rc)
    rc = search_enqueue(b, (const orbfe_kf_point*)(b->d_stage + st.o_pts), n_points, partial ? (const int32_t*)(b->d_stage + st.o_idx) : nullptr,
                        n_idx, first_target, skip ? b->d_stage + st.o_skip : nullptr, (orbfe_kf_result*)(b->d_stage + st.o_res), first_target,
                        n_rec, 1, b->stream);
  if (!rc && b_res) rc = hip_status("orbfe_fuse_batch_search", hipMemcpyAsync(b->h_stage + st.o_res, b->d_stage + st.o_res, b_res, hipMemcpyDeviceToHost, b->stream));
  const hipError_t e2 = hipStreamSynchronize(b->stream);   // also on an error: the stream may still read the pinned block
  if (!rc) rc = hip_status("orbfe_fuse_batch_search", e2);
  if (rc) return rc;
  orbfe_fuse_unstage_results((const orbfe_kf_result*)(b->h_stage + st.o_res), b->K, n_points, point_idx, n_rec, first_target, results);
  return ORBFE_OK;
}
