// initial_map.cpp -- C ABI of Tracking::CreateInitialMapMonocular (include/orbfe.h: orbfe_create_initial_map,
// orbfe_create_initial_map_batch_device, orbfe_initial_map_workspace_bytes).  The entry points validate, stage and launch
// initial_map_kernels.hip.  No CPU fallback: without a device both forms are an error.
#include <string.h>

#include "host_internal.h"
#include "initial_map_internal.h"

static bool caps_ok(int P, int cap) {
  if (P < 0 || P > ORBFE_LBA_MAX_PROBLEMS || cap < 1 || cap > ORBFE_INIT_MAX_MATCHES) {
    orbfe_set_error("create initial map: P %d (0 .. %d), cap %d (1 .. %d)", P, ORBFE_LBA_MAX_PROBLEMS, cap, ORBFE_INIT_MAX_MATCHES);
    return false;
  }
  return true;
}

static bool rules_ok(int n_iterations, int q, int min_points) {
  if (n_iterations < 1 || n_iterations > ORBFE_BA_MAX_ITERATIONS || q < 1 || min_points < 0) {
    orbfe_set_error("create initial map: n_iterations %d (1 .. %d), q %d (>= 1), min_points %d (>= 0)", n_iterations,
                    ORBFE_BA_MAX_ITERATIONS, q, min_points);
    return false;
  }
  return true;
}

extern "C" int orbfe_initial_map_workspace_bytes(int P, int cap, size_t* bytes) {
  if (!bytes) {
    orbfe_set_error("initial map workspace bytes: bytes is required");
    return ORBFE_ERR_INVALID;
  }
  if (!caps_ok(P, cap)) return ORBFE_ERR_INVALID;
  *bytes = imap_ws_carve(nullptr, P, cap, nullptr);
  return ORBFE_OK;
}

extern "C" int orbfe_create_initial_map_batch_device(int P, const orbfe_pose_camera* d_camera, const float* d_keys1, const int32_t* d_n1,
                                                     const float* d_keys2, const int32_t* d_n2, int cap, const int32_t* d_matches12,
                                                     const float* d_P3D, const uint64_t* d_triangulated, const orbfe_init_result* d_init,
                                                     const int32_t* d_octaves1, const int32_t* d_octaves2, const float* d_pose1,
                                                     int n_iterations, int q, int min_points, float* d_poses, float* d_points,
                                                     int32_t* d_index, float* d_poses_ba, float* d_points_ba,
                                                     orbfe_initial_map_result* d_result, void* d_workspace, size_t workspace_bytes,
                                                     void* stream) {
  if (!caps_ok(P, cap) || !rules_ok(n_iterations, q, min_points)) return ORBFE_ERR_INVALID;
  if (!d_camera || !d_keys1 || !d_n1 || !d_keys2 || !d_n2 || !d_matches12 || !d_P3D || !d_triangulated || !d_init || !d_octaves1 ||
      !d_octaves2 || !d_poses || !d_points || !d_index || !d_result) {
    orbfe_set_error("create initial map batch: every pointer but d_pose1, d_poses_ba and d_points_ba is required");
    return ORBFE_ERR_INVALID;
  }
  const uintptr_t four = (uintptr_t)d_camera | (uintptr_t)d_keys1 | (uintptr_t)d_n1 | (uintptr_t)d_keys2 | (uintptr_t)d_n2 |
                         (uintptr_t)d_matches12 | (uintptr_t)d_P3D | (uintptr_t)d_init | (uintptr_t)d_octaves1 | (uintptr_t)d_octaves2 |
                         (uintptr_t)d_pose1 | (uintptr_t)d_poses | (uintptr_t)d_points | (uintptr_t)d_index | (uintptr_t)d_poses_ba |
                         (uintptr_t)d_points_ba;
  if ((four & 3) || ((uintptr_t)d_triangulated & 7) || ((uintptr_t)d_result & 7)) {
    orbfe_set_error("create initial map batch: records must be 4-byte aligned, d_triangulated and d_result 8-byte");
    return ORBFE_ERR_INVALID;
  }
  const size_t need = imap_ws_carve(nullptr, P, cap, nullptr);
  if (need > 0 && (!d_workspace || workspace_bytes < need || ((uintptr_t)d_workspace & 255))) {
    orbfe_set_error("create initial map batch: the workspace needs %zu bytes at a 256-byte boundary (%zu given)", need, workspace_bytes);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (P == 0) return ORBFE_OK;
  ImapLaunch L;
  memset(&L, 0, sizeof(L));
  L.camera = d_camera; L.keys1 = d_keys1; L.keys2 = d_keys2; L.n1 = d_n1; L.n2 = d_n2; L.cap = cap; L.matches12 = d_matches12;
  L.P3D = d_P3D; L.triangulated = d_triangulated; L.init = d_init; L.octaves1 = d_octaves1; L.octaves2 = d_octaves2; L.pose1 = d_pose1;
  L.n_iterations = n_iterations; L.q = q; L.min_points = min_points; L.poses = d_poses; L.points = d_points; L.index = d_index;
  L.poses_ba = d_poses_ba; L.points_ba = d_points_ba; L.result = d_result;
  imap_ws_carve((uint8_t*)d_workspace, P, cap, &L);
  orbfe_launch_initial_map(L, P, (hipStream_t)stream);
  return hip_status("create initial map batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_create_initial_map(const orbfe_pose_camera* camera, const float* keys1, int n1, const float* keys2, int n2,
                                        const int32_t* matches12, const float* P3D, const uint64_t* triangulated,
                                        const orbfe_init_result* init, const int32_t* octaves1, const int32_t* octaves2, const float* pose1,
                                        int n_iterations, int q, int min_points, float* poses, float* points, int32_t* index,
                                        float* poses_ba, float* points_ba, orbfe_initial_map_result* result) {
  if (!camera || !init || !poses || !result) {
    orbfe_set_error("create initial map: camera, init, poses and result are required");
    return ORBFE_ERR_INVALID;
  }
  if (n1 < 0 || n1 > ORBFE_INIT_MAX_MATCHES || n2 < 0 || n2 > ORBFE_INIT_MAX_MATCHES) {
    orbfe_set_error("create initial map: n1 %d, n2 %d (0 .. %d)", n1, n2, ORBFE_INIT_MAX_MATCHES);
    return ORBFE_ERR_INVALID;
  }
  if (!rules_ok(n_iterations, q, min_points)) return ORBFE_ERR_INVALID;
  if ((n1 > 0 && (!keys1 || !matches12 || !P3D || !triangulated || !octaves1 || !points || !index)) || (n2 > 0 && (!keys2 || !octaves2))) {
    orbfe_set_error("create initial map: the arrays of a count > 0 are required");
    return ORBFE_ERR_INVALID;
  }
  if (camera->n_levels < 1 || camera->n_levels > ORBFE_MAX_LEVELS) {
    orbfe_set_error("create initial map: camera.n_levels %d (1 .. %d)", camera->n_levels, ORBFE_MAX_LEVELS);
    return ORBFE_ERR_INVALID;
  }
  for (int i = 0; i < n1; i++) {
    const int32_t m = matches12[i];
    if (m >= n2) {
      orbfe_set_error("create initial map: matches12[%d] = %d (< n2 = %d)", i, m, n2);
      return ORBFE_ERR_INVALID;
    }
    if (!imap_is_point(m, n2, triangulated[i >> 6], i & 63)) continue;
    if (octaves1[i] < 0 || octaves1[i] >= camera->n_levels || octaves2[m] < 0 || octaves2[m] >= camera->n_levels) {
      orbfe_set_error("create initial map: match %d -> %d: octaves %d and %d (0 .. %d)", i, m, octaves1[i], octaves2[m],
                      camera->n_levels - 1);
      return ORBFE_ERR_INVALID;
    }
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;

  // the workspace is an allocation of its own; its guard is declared before the call, so it is freed after the call has drained
  struct Workspace {
    void* p = nullptr;
    ~Workspace() {
      if (p) (void)hipFree(p);
    }
  } ws;
  const int cap = n1 > n2 ? (n1 > 0 ? n1 : 1) : (n2 > 0 ? n2 : 1), W = (cap + 63) >> 6;
  HostCall c("create initial map");
  const size_t o_cam = c.in(sizeof(orbfe_pose_camera)), o_k1 = c.in((size_t)cap * 8), o_k2 = c.in((size_t)cap * 8), o_n = c.in(8),
               o_m = c.in((size_t)cap * 4), o_p3d = c.in((size_t)cap * 12), o_tri = c.in((size_t)W * 8), o_init = c.in(sizeof(orbfe_init_result)),
               o_o1 = c.in((size_t)cap * 4), o_o2 = c.in((size_t)cap * 4), o_pose1 = c.in(48);
  const size_t o_res = c.out(sizeof(orbfe_initial_map_result)), o_poses = c.out(96), o_poses_ba = c.out(96), o_index = c.out((size_t)cap * 4),
               o_points = c.out((size_t)cap * 12), o_points_ba = c.out((size_t)cap * 12);
  const size_t ws_bytes = imap_ws_carve(nullptr, 1, cap, nullptr);
  int rc;
  if ((rc = c.open())) return rc;
  if ((rc = hip_status("create initial map: workspace", hipMalloc(&ws.p, ws_bytes)))) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  memcpy(h + o_cam, camera, sizeof(orbfe_pose_camera));
  const int32_t counts[2] = {n1, n2};
  memcpy(h + o_n, counts, 8);
  memset(h + o_tri, 0, (size_t)W * 8);
  if (n1) {
    memcpy(h + o_k1, keys1, (size_t)n1 * 8);
    memcpy(h + o_m, matches12, (size_t)n1 * 4);
    memcpy(h + o_p3d, P3D, (size_t)n1 * 12);
    memcpy(h + o_tri, triangulated, (size_t)((n1 + 63) >> 6) * 8);
    memcpy(h + o_o1, octaves1, (size_t)n1 * 4);
  }
  if (n2) {
    memcpy(h + o_k2, keys2, (size_t)n2 * 8);
    memcpy(h + o_o2, octaves2, (size_t)n2 * 4);
  }
  memcpy(h + o_init, init, sizeof(orbfe_init_result));
  if (pose1) memcpy(h + o_pose1, pose1, 48);
  if ((rc = c.upload())) return rc;
  ImapLaunch L;
  memset(&L, 0, sizeof(L));
  L.camera = (const orbfe_pose_camera*)(d + o_cam); L.keys1 = (const float*)(d + o_k1); L.keys2 = (const float*)(d + o_k2);
  L.n1 = (const int32_t*)(d + o_n); L.n2 = (const int32_t*)(d + o_n) + 1; L.cap = cap; L.matches12 = (const int32_t*)(d + o_m);
  L.P3D = (const float*)(d + o_p3d); L.triangulated = (const uint64_t*)(d + o_tri); L.init = (const orbfe_init_result*)(d + o_init);
  L.octaves1 = (const int32_t*)(d + o_o1); L.octaves2 = (const int32_t*)(d + o_o2); L.pose1 = pose1 ? (const float*)(d + o_pose1) : nullptr;
  L.n_iterations = n_iterations; L.q = q; L.min_points = min_points; L.poses = (float*)(d + o_poses); L.points = (float*)(d + o_points);
  L.index = (int32_t*)(d + o_index); L.poses_ba = (float*)(d + o_poses_ba); L.points_ba = (float*)(d + o_points_ba);
  L.result = (orbfe_initial_map_result*)(d + o_res);
  imap_ws_carve((uint8_t*)ws.p, 1, cap, &L);
  orbfe_launch_initial_map(L, 1, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(result, h + o_res, sizeof(*result));
  memcpy(poses, h + o_poses, 96);
  if (poses_ba) memcpy(poses_ba, h + o_poses_ba, 96);
  if (n1) {
    memcpy(index, h + o_index, (size_t)n1 * 4);
    memcpy(points, h + o_points, (size_t)n1 * 12);
    if (points_ba) memcpy(points_ba, h + o_points_ba, (size_t)n1 * 12);
  }
  return ORBFE_OK;
}
