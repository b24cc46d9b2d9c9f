// lba.cpp -- C ABI of Optimizer::LocalBundleAdjustment (include/orbfe.h: orbfe_local_bundle_adjustment,
// orbfe_local_bundle_adjustment_batch_device, orbfe_lba_workspace_bytes).  The entry points validate, stage and launch
// lba_kernels.hip.  No CPU fallback: without a device both forms are an error.
// Optimizer::BundleAdjustment (ba.cpp) is the same graph under another schedule: what the two share of validating, sorting, staging
// and launching is lba_batch_entry and lba_host_entry here, told apart by LbaSchedule (lba_internal.h).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "host_internal.h"
#include "lba_internal.h"

static const LbaSchedule LOCAL = {"local bundle adjustment", 0, ORBFE_LBA_FIRST_ROUND_ONLY};

static bool caps_ok(const char* who, int P, int kf_cap, int point_cap, int edge_cap) {
  if (P < 0 || P > ORBFE_LBA_MAX_PROBLEMS || kf_cap < 0 || kf_cap > ORBFE_LBA_MAX_KEYFRAMES || point_cap < 0 ||
      point_cap > ORBFE_LBA_MAX_POINTS || edge_cap < 0 || edge_cap > ORBFE_LBA_MAX_EDGES) {
    orbfe_set_error("%s: P %d (0 .. %d), kf_cap %d (0 .. %d), point_cap %d (0 .. %d), edge_cap %d (0 .. %d)", who, P,
                    ORBFE_LBA_MAX_PROBLEMS, kf_cap, ORBFE_LBA_MAX_KEYFRAMES, point_cap, ORBFE_LBA_MAX_POINTS, edge_cap,
                    ORBFE_LBA_MAX_EDGES);
    return false;
  }
  return true;
}

static size_t problem_bytes(int kf_cap, int point_cap, int edge_cap) {
  return lba_ws_bytes(std::min(kf_cap, ORBFE_LBA_MAX_FREE), point_cap, edge_cap);
}

extern "C" int orbfe_lba_workspace_bytes(int P, int kf_cap, int point_cap, int edge_cap, size_t* bytes) {
  if (!bytes) {
    orbfe_set_error("lba workspace bytes: bytes is required");
    return ORBFE_ERR_INVALID;
  }
  if (!caps_ok(LOCAL.who, P, kf_cap, point_cap, edge_cap)) return ORBFE_ERR_INVALID;
  *bytes = (size_t)P * problem_bytes(kf_cap, point_cap, edge_cap);
  return ORBFE_OK;
}

// ", n_iterations N (1 .. cap)" for the schedule that has such an argument, nothing for the one that has not
static std::string iterations_text(const LbaSchedule& S) {
  if (!S.ba) return "";
  return ", n_iterations " + std::to_string(S.n_iterations) + " (1 .. " + std::to_string(ORBFE_BA_MAX_ITERATIONS) + ")";
}

static bool schedule_ok(const LbaSchedule& S, int flags) {
  return !(flags & ~S.known_flags) && (!S.ba || (S.n_iterations >= 1 && S.n_iterations <= ORBFE_BA_MAX_ITERATIONS));
}

// launches the schedule's kernel; result: orbfe_lba_result, or orbfe_ba_result for Optimizer::BundleAdjustment
static void launch(const LbaSchedule& S, LbaLaunch& L, void* result, int P, hipStream_t stream) {
  if (S.ba) {
    orbfe_launch_ba(L, S.n_iterations, (orbfe_ba_result*)result, P, stream);
  } else {
    L.result = (orbfe_lba_result*)result;
    orbfe_launch_lba(L, P, stream);
  }
}

int lba_batch_entry(const LbaSchedule& S, int P, const orbfe_pose_camera* d_camera, const orbfe_lba_problem* d_problems,
                    const float* d_poses, const uint8_t* d_fixed, const uint8_t* d_points, int point_stride, const orbfe_lba_edge* d_edges,
                    int kf_cap, int point_cap, int edge_cap, int flags, float* d_poses_out, float* d_points_out, uint8_t* d_erase,
                    void* d_result, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!caps_ok(S.who, P, kf_cap, point_cap, edge_cap)) return ORBFE_ERR_INVALID;
  if (point_stride < 12 || (point_stride & 3) || !schedule_ok(S, flags)) {
    orbfe_set_error("%s batch: point_stride %d (>= 12, a multiple of 4), flags %d%s", S.who, point_stride, flags, iterations_text(S).c_str());
    return ORBFE_ERR_INVALID;
  }
  if (!d_camera || !d_problems || !d_result || (kf_cap > 0 && (!d_poses || !d_fixed || !d_poses_out)) ||
      (point_cap > 0 && (!d_points || !d_points_out)) || (edge_cap > 0 && (!d_edges || (!S.ba && !d_erase)))) {
    orbfe_set_error("%s batch: every pointer is required (the arrays of a cap of 0 may be null)", S.who);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_camera & 3) || ((uintptr_t)d_problems & 3) || ((uintptr_t)d_poses & 3) || ((uintptr_t)d_points & 3) ||
      ((uintptr_t)d_edges & 3) || ((uintptr_t)d_poses_out & 3) || ((uintptr_t)d_points_out & 3) || ((uintptr_t)d_result & 7)) {
    orbfe_set_error("%s batch: records must be 4-byte aligned, d_result 8-byte", S.who);
    return ORBFE_ERR_INVALID;
  }
  const size_t need = (size_t)P * problem_bytes(kf_cap, point_cap, edge_cap);
  if (need > 0 && (!d_workspace || workspace_bytes < need || ((uintptr_t)d_workspace & 255))) {
    orbfe_set_error("%s batch: the workspace needs %zu bytes at a 256-byte boundary (%zu given)", S.who, need, workspace_bytes);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (P == 0) return ORBFE_OK;
  LbaLaunch L;
  memset(&L, 0, sizeof(L));
  L.camera = d_camera; L.problems = d_problems; L.poses = d_poses; L.fixed = d_fixed; L.points = d_points; L.point_stride = point_stride;
  L.edges = d_edges; L.kf_cap = kf_cap; L.point_cap = point_cap; L.edge_cap = edge_cap; L.flags = flags; L.poses_out = d_poses_out;
  L.points_out = d_points_out; L.erase = d_erase; L.workspace = (uint8_t*)d_workspace;
  launch(S, L, d_result, P, (hipStream_t)stream);
  return hip_status((std::string(S.who) + " batch: kernel launch failed").c_str(), hipGetLastError());
}

extern "C" int orbfe_local_bundle_adjustment_batch_device(int P, const orbfe_pose_camera* d_camera, const orbfe_lba_problem* d_problems,
                                                          const float* d_poses, const uint8_t* d_fixed, const uint8_t* d_points,
                                                          int point_stride, const orbfe_lba_edge* d_edges, int kf_cap, int point_cap,
                                                          int edge_cap, int flags, float* d_poses_out, float* d_points_out,
                                                          uint8_t* d_erase, orbfe_lba_result* d_result, void* d_workspace,
                                                          size_t workspace_bytes, void* stream) {
  return lba_batch_entry(LOCAL, P, d_camera, d_problems, d_poses, d_fixed, d_points, point_stride, d_edges, kf_cap, point_cap, edge_cap,
                         flags, d_poses_out, d_points_out, d_erase, d_result, d_workspace, workspace_bytes, stream);
}

int lba_host_entry(const LbaSchedule& S, const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf,
                   const float* points, int n_points, const orbfe_lba_edge* edges, int n_edges, int flags, float* poses_out,
                   float* points_out, uint8_t* erase, void* result) {
  const size_t result_bytes = S.ba ? sizeof(orbfe_ba_result) : sizeof(orbfe_lba_result);
  if (!camera || !result) {
    orbfe_set_error("%s: camera and result are required", S.who);
    return ORBFE_ERR_INVALID;
  }
  if (n_kf < 0 || n_points < 0 || n_edges < 0 || !schedule_ok(S, flags)) {
    orbfe_set_error("%s: n_kf %d, n_points %d, n_edges %d (>= 0), flags %d%s", S.who, n_kf, n_points, n_edges, flags,
                    iterations_text(S).c_str());
    return ORBFE_ERR_INVALID;
  }
  if (!caps_ok(S.who, 1, n_kf, n_points, n_edges)) return ORBFE_ERR_INVALID;
  if ((n_kf > 0 && (!poses || !fixed || !poses_out)) || (n_points > 0 && (!points || !points_out)) ||
      (n_edges > 0 && (!edges || (!S.ba && !erase)))) {
    orbfe_set_error("%s: the arrays of a count > 0 are required", S.who);
    return ORBFE_ERR_INVALID;
  }
  int n_free = 0;
  for (int k = 0; k < n_kf; k++) n_free += fixed[k] ? 0 : 1;
  if (n_free > ORBFE_LBA_MAX_FREE) {
    orbfe_set_error("%s: %d free keyframes (0 .. %d)", S.who, n_free, ORBFE_LBA_MAX_FREE);
    return ORBFE_ERR_INVALID;
  }
  for (int i = 0; i < n_edges; i++) {
    const orbfe_lba_edge& E = edges[i];
    if (E.kf < 0 || E.kf >= n_kf || E.point < 0 || E.point >= n_points || !(E.inv_sigma2 > 0.0f) || !isfinite(E.inv_sigma2)) {
      orbfe_set_error("%s: edge %d: kf %d (0 .. %d), point %d (0 .. %d), inv_sigma2 %g (finite, > 0)", S.who, i, E.kf,
                      n_kf - 1, E.point, n_points - 1, (double)E.inv_sigma2);
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
      orbfe_set_error("%s: edges %d and %d join the same keyframe %d and point %d", S.who, order[j - 1], order[j],
                      edges[order[j]].kf, edges[order[j]].point);
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
  HostCall c(S.who);
  const size_t o_cam = c.in(sizeof(orbfe_pose_camera)), o_prob = c.in(sizeof(orbfe_lba_problem)), o_poses = c.in((size_t)n_kf * 48),
               o_fixed = c.in((size_t)n_kf), o_points = c.in((size_t)n_points * 12), o_edges = c.in((size_t)n_edges * sizeof(orbfe_lba_edge));
  const size_t o_res = c.out(result_bytes), o_pout = c.out((size_t)n_kf * 48), o_xout = c.out((size_t)n_points * 12),
               o_erase = c.out((size_t)n_edges);
  const size_t ws_bytes = problem_bytes(n_kf, n_points, n_edges);
  int rc;
  if ((rc = c.open())) return rc;
  if (ws_bytes && (rc = hip_status((std::string(S.who) + ": workspace").c_str(), hipMalloc(&ws.p, ws_bytes)))) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  memcpy(h + o_cam, camera, sizeof(orbfe_pose_camera));
  const orbfe_lba_problem prob = {0, n_kf, 0, n_points, 0, n_edges};
  memcpy(h + o_prob, &prob, sizeof(prob));
  if (n_kf) memcpy(h + o_poses, poses, (size_t)n_kf * 48);
  if (n_kf) memcpy(h + o_fixed, fixed, (size_t)n_kf);
  if (n_points) memcpy(h + o_points, points, (size_t)n_points * 12);
  orbfe_lba_edge* he = (orbfe_lba_edge*)(h + o_edges);
  for (int j = 0; j < n_edges; j++) he[j] = edges[order[j]];
  if ((rc = c.upload())) return rc;
  LbaLaunch L;
  memset(&L, 0, sizeof(L));
  L.camera = (const orbfe_pose_camera*)(d + o_cam); L.problems = (const orbfe_lba_problem*)(d + o_prob);
  L.poses = (const float*)(d + o_poses); L.fixed = d + o_fixed; L.points = d + o_points; L.point_stride = 12;
  L.edges = (const orbfe_lba_edge*)(d + o_edges); L.kf_cap = n_kf; L.point_cap = n_points; L.edge_cap = n_edges; L.flags = flags;
  L.poses_out = (float*)(d + o_pout); L.points_out = (float*)(d + o_xout); L.erase = d + o_erase;
  L.workspace = (uint8_t*)ws.p;
  launch(S, L, d + o_res, 1, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(result, h + o_res, result_bytes);
  if (n_kf) memcpy(poses_out, h + o_pout, (size_t)n_kf * 48);
  if (n_points) memcpy(points_out, h + o_xout, (size_t)n_points * 12);
  if (!S.ba)
    for (int j = 0; j < n_edges; j++) erase[order[j]] = h[o_erase + j];
  return ORBFE_OK;
}

extern "C" int orbfe_local_bundle_adjustment(const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf,
                                             const float* points, int n_points, const orbfe_lba_edge* edges, int n_edges, int flags,
                                             float* poses_out, float* points_out, uint8_t* erase, orbfe_lba_result* result) {
  return lba_host_entry(LOCAL, camera, poses, fixed, n_kf, points, n_points, edges, n_edges, flags, poses_out, points_out, erase, result);
}
