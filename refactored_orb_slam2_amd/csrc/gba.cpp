// gba.cpp -- C ABI of the global bundle adjustment across the device (include/orbfe.h: orbfe_global_bundle_adjustment,
// orbfe_gba_workspace_bytes, orbfe_global_bundle_adjustment_device).  The entry points validate against the ORBFE_GBA_MAX_* limits
// before any device is looked for, sort and stage (HostCall) as lba.cpp does for the one-workgroup form, and hand the problem to
// the host loop of gba_kernels.hip.  No CPU fallback: without a device both forms are an error.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "host_internal.h"
#include "gba_internal.h"

static const char* WHO = "global bundle adjustment";

static bool counts_ok(int n_kf, int n_points, int n_edges) {
  if (n_kf < 0 || n_kf > ORBFE_GBA_MAX_KEYFRAMES || n_points < 0 || n_points > ORBFE_GBA_MAX_POINTS || n_edges < 0 ||
      n_edges > ORBFE_GBA_MAX_EDGES) {
    orbfe_set_error("%s: n_kf %d (0 .. %d), n_points %d (0 .. %d), n_edges %d (0 .. %d)", WHO, n_kf, ORBFE_GBA_MAX_KEYFRAMES, n_points,
                    ORBFE_GBA_MAX_POINTS, n_edges, ORBFE_GBA_MAX_EDGES);
    return false;
  }
  return true;
}

static bool schedule_ok(int n_iterations, int flags) {
  if ((flags & ~ORBFE_BA_ROBUST) || n_iterations < 1 || n_iterations > ORBFE_BA_MAX_ITERATIONS) {
    orbfe_set_error("%s: flags %d, n_iterations %d (1 .. %d)", WHO, flags, n_iterations, ORBFE_BA_MAX_ITERATIONS);
    return false;
  }
  return true;
}

extern "C" int orbfe_gba_workspace_bytes(int kf_cap, int point_cap, int edge_cap, size_t* bytes) {
  if (!bytes) {
    orbfe_set_error("%s: workspace bytes: bytes is required", WHO);
    return ORBFE_ERR_INVALID;
  }
  if (!counts_ok(kf_cap, point_cap, edge_cap)) return ORBFE_ERR_INVALID;
  *bytes = gba_ws_bytes(kf_cap, point_cap, edge_cap);
  return ORBFE_OK;
}

// the control record's pinned mirror, for the length of one call
struct PinnedControl {
  GbaControl* p = nullptr;
  ~PinnedControl() {
    if (p) (void)hipHostFree(p);
  }
};

// orbfe_debug_gba_phases: the calling thread's switch and its sums of stream-event times per phase
static thread_local bool t_timing = false;
static thread_local float t_phase_ms[GBA_PHASES];

extern "C" int orbfe_debug_gba_phases(int enable, float* ms) {
  if (ms) memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  memset(t_phase_ms, 0, sizeof(t_phase_ms));
  t_timing = enable != 0;
  return ORBFE_OK;
}

static int run(const GbaLaunch& L, void* d_workspace, hipStream_t stream) {
  PinnedControl pc;
  int rc;
  if ((rc = hip_status("global bundle adjustment: control record", hipHostMalloc((void**)&pc.p, sizeof(GbaControl), hipHostMallocDefault))))
    return rc;
  GbaWs G;
  gba_ws_carve((uint8_t*)d_workspace, L.n_kf, L.n_points, L.n_edges, G);
  return hip_status("global bundle adjustment: launch", orbfe_run_gba(L, G, pc.p, stream, t_timing ? t_phase_ms : nullptr));
}

extern "C" int orbfe_global_bundle_adjustment_device(const orbfe_pose_camera* d_camera, const float* d_poses, const uint8_t* d_fixed,
                                                     int n_kf, const uint8_t* d_points, int point_stride, int n_points,
                                                     const orbfe_lba_edge* d_edges, int n_edges, int n_iterations, int flags,
                                                     float* d_poses_out, float* d_points_out, orbfe_ba_result* d_result,
                                                     void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!counts_ok(n_kf, n_points, n_edges) || !schedule_ok(n_iterations, flags)) return ORBFE_ERR_INVALID;
  if (point_stride < 12 || (point_stride & 3)) {
    orbfe_set_error("%s device: point_stride %d (>= 12, a multiple of 4)", WHO, point_stride);
    return ORBFE_ERR_INVALID;
  }
  if (!d_camera || !d_result || (n_kf > 0 && (!d_poses || !d_fixed || !d_poses_out)) || (n_points > 0 && (!d_points || !d_points_out)) ||
      (n_edges > 0 && !d_edges)) {
    orbfe_set_error("%s device: every pointer is required (the arrays of a count of 0 may be null)", WHO);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_camera & 3) || ((uintptr_t)d_poses & 3) || ((uintptr_t)d_points & 3) || ((uintptr_t)d_edges & 3) ||
      ((uintptr_t)d_poses_out & 3) || ((uintptr_t)d_points_out & 3) || ((uintptr_t)d_result & 7)) {
    orbfe_set_error("%s device: records must be 4-byte aligned, d_result 8-byte", WHO);
    return ORBFE_ERR_INVALID;
  }
  const size_t need = gba_ws_bytes(n_kf, n_points, n_edges);
  if (!d_workspace || workspace_bytes < need || ((uintptr_t)d_workspace & 255)) {
    orbfe_set_error("%s device: the workspace needs %zu bytes at a 256-byte boundary (%zu given)", WHO, need, workspace_bytes);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  GbaLaunch L;
  memset(&L, 0, sizeof(L));
  L.camera = d_camera; L.poses = d_poses; L.fixed = d_fixed; L.points = d_points; L.point_stride = point_stride; L.edges = d_edges;
  L.n_kf = n_kf; L.n_points = n_points; L.n_edges = n_edges; L.n_iterations = n_iterations; L.flags = flags;
  L.poses_out = d_poses_out; L.points_out = d_points_out; L.result = d_result;
  return run(L, d_workspace, (hipStream_t)stream);
}

extern "C" int orbfe_global_bundle_adjustment(const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf,
                                              const float* points, int n_points, const orbfe_lba_edge* edges, int n_edges,
                                              int n_iterations, int flags, float* poses_out, float* points_out, orbfe_ba_result* result) {
  if (!camera || !result) {
    orbfe_set_error("%s: camera and result are required", WHO);
    return ORBFE_ERR_INVALID;
  }
  if (!counts_ok(n_kf, n_points, n_edges) || !schedule_ok(n_iterations, flags)) return ORBFE_ERR_INVALID;
  if ((n_kf > 0 && (!poses || !fixed || !poses_out)) || (n_points > 0 && (!points || !points_out)) || (n_edges > 0 && !edges)) {
    orbfe_set_error("%s: the arrays of a count > 0 are required", WHO);
    return ORBFE_ERR_INVALID;
  }
  for (int i = 0; i < n_edges; i++) {
    const orbfe_lba_edge& E = edges[i];
    if (E.kf < 0 || E.kf >= n_kf || E.point < 0 || E.point >= n_points || !(E.inv_sigma2 > 0.0f) || !isfinite(E.inv_sigma2)) {
      orbfe_set_error("%s: edge %d: kf %d (0 .. %d), point %d (0 .. %d), inv_sigma2 %g (finite, > 0)", WHO, i, E.kf, n_kf - 1, E.point,
                      n_points - 1, (double)E.inv_sigma2);
      return ORBFE_ERR_INVALID;
    }
  }
  // the plan's order: point by point, keyframes ascending; order[j] = the caller's row of sorted edge j
  std::vector<int32_t> order(n_edges);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [edges](int32_t a, int32_t b) {
    return edges[a].point != edges[b].point ? edges[a].point < edges[b].point : edges[a].kf < edges[b].kf;
  });
  for (int j = 1; j < n_edges; j++)
    if (edges[order[j]].point == edges[order[j - 1]].point && edges[order[j]].kf == edges[order[j - 1]].kf) {
      orbfe_set_error("%s: edges %d and %d join the same keyframe %d and point %d", WHO, order[j - 1], order[j], edges[order[j]].kf,
                      edges[order[j]].point);
      return ORBFE_ERR_INVALID;
    }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;

  // the workspace is an allocation of its own; its guard is declared before the call, so it is freed after the call has drained
  struct Workspace {
    void* p = nullptr;
    ~Workspace() {
      if (p) (void)hipFree(p);
    }
  } ws;
  HostCall c(WHO);
  const size_t o_cam = c.in(sizeof(orbfe_pose_camera)), o_poses = c.in((size_t)n_kf * 48), o_fixed = c.in((size_t)n_kf),
               o_points = c.in((size_t)n_points * 12), o_edges = c.in((size_t)n_edges * sizeof(orbfe_lba_edge));
  const size_t o_res = c.out(sizeof(orbfe_ba_result)), o_pout = c.out((size_t)n_kf * 48), o_xout = c.out((size_t)n_points * 12);
  int rc;
  if ((rc = c.open())) return rc;
  if ((rc = hip_status("global bundle adjustment: workspace", hipMalloc(&ws.p, gba_ws_bytes(n_kf, n_points, n_edges))))) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  memcpy(h + o_cam, camera, sizeof(orbfe_pose_camera));
  if (n_kf) memcpy(h + o_poses, poses, (size_t)n_kf * 48);
  if (n_kf) memcpy(h + o_fixed, fixed, (size_t)n_kf);
  if (n_points) memcpy(h + o_points, points, (size_t)n_points * 12);
  orbfe_lba_edge* he = (orbfe_lba_edge*)(h + o_edges);
  for (int j = 0; j < n_edges; j++) he[j] = edges[order[j]];
  if ((rc = c.upload())) return rc;
  GbaLaunch L;
  memset(&L, 0, sizeof(L));
  L.camera = (const orbfe_pose_camera*)(d + o_cam); L.poses = (const float*)(d + o_poses); L.fixed = d + o_fixed; L.points = d + o_points;
  L.point_stride = 12; L.edges = (const orbfe_lba_edge*)(d + o_edges); L.n_kf = n_kf; L.n_points = n_points; L.n_edges = n_edges;
  L.n_iterations = n_iterations; L.flags = flags; L.poses_out = (float*)(d + o_pout); L.points_out = (float*)(d + o_xout);
  L.result = (orbfe_ba_result*)(d + o_res);
  if ((rc = run(L, ws.p, c.stream))) return rc;
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(result, h + o_res, sizeof(orbfe_ba_result));
  if (n_kf) memcpy(poses_out, h + o_pout, (size_t)n_kf * 48);
  if (n_points) memcpy(points_out, h + o_xout, (size_t)n_points * 12);
  return ORBFE_OK;
}
