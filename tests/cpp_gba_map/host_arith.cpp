// host_arith.cpp -- csrc/gba_map_internal.h, with the headers under it, compiled for the HOST: the items gba_map_kernels.hip hands to
// its lanes, in plain loops, so that the arithmetic the kernels execute can be compared with the numpy yardstick on a machine without
// a GPU (tests/test_gba_map_cpu.py).  Same flags as the library (-ffp-contract=off).
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/gba_map_internal.h"

// SetPose's Twc (12 floats) and Cw (3) of n poses
extern "C" void gba_map_host_set_pose(const float* Tcw, int n, float half_baseline, float* Twc, float* Cw) {
  for (int k = 0; k < n; k++) gm_set_pose(Tcw + 12 * (size_t)k, half_baseline, Twc + 12 * (size_t)k, Cw + 3 * (size_t)k);
}

// C[k] = A[k] * B[k] of n pairs of 4 x 4 operands
extern "C" void gba_map_host_mul(const float* A, const float* B, int n, float* C) {
  for (int k = 0; k < n; k++) gm_mul(A + 12 * (size_t)k, B + 12 * (size_t)k, C + 12 * (size_t)k);
}

// The whole update with the rules of the device form, rows out of range included: the prepare step per keyframe, sweeps over the
// pending keyframes against the marks of the sweep before until one sets none, the finish step, the points
extern "C" void gba_map_host_update(const float* poses, const int32_t* parent, const int32_t* kf_gba_row, int n_kf, const float* gba_poses,
                                    int n_gba_kf, float hb, const float* points, const int32_t* point_gba_row, const int32_t* ref,
                                    int n_points, const float* gba_points, int n_gba_points, orbfe_gba_map_keyframe* kf_out,
                                    float* points_out, orbfe_gba_map_result* result) {
  memset(result, 0, sizeof(*result));
  std::vector<uint8_t> done(n_kf, 0), earned(n_kf, 0);
  for (int k = 0; k < n_kf; k++) {
    orbfe_gba_map_keyframe& rec = kf_out[k];
    const int row = kf_gba_row[k], par = parent[k];
    if (row >= 0 && row < n_gba_kf) {
      memcpy(rec.Tcw, gba_poses + 12 * (size_t)row, 48);
      rec.status = ORBFE_GBA_MAP_KF_OPTIMISED;
      done[k] = 1;
    } else if (row < 0 && par >= 0 && par < n_kf) {
      gm_relative(poses + 12 * (size_t)k, poses + 12 * (size_t)par, hb, rec.Tcw);
      rec.status = GM_PENDING;
    } else {
      rec.status = ORBFE_GBA_MAP_KF_UNREACHED;
    }
  }
  for (;;) {
    bool any = false;
    for (int k = 0; k < n_kf; k++) {
      if (kf_out[k].status != GM_PENDING || !done[parent[k]]) continue;
      float T[12];
      gm_propagate(kf_out[k].Tcw, kf_out[parent[k]].Tcw, T);
      memcpy(kf_out[k].Tcw, T, 48);
      kf_out[k].status = ORBFE_GBA_MAP_KF_PROPAGATED;
      earned[k] = 1;
      any = true;
    }
    if (!any) break;
    for (int k = 0; k < n_kf; k++)
      if (earned[k]) done[k] = 1, earned[k] = 0;
    result->rounds++;
  }
  for (int k = 0; k < n_kf; k++) {
    orbfe_gba_map_keyframe& rec = kf_out[k];
    if (rec.status == GM_PENDING) rec.status = ORBFE_GBA_MAP_KF_UNREACHED;
    if (rec.status == ORBFE_GBA_MAP_KF_UNREACHED) memcpy(rec.Tcw, poses + 12 * (size_t)k, 48);
    gm_set_pose(rec.Tcw, hb, rec.Twc, rec.Cw);
    (&result->n_optimised)[rec.status]++;
  }
  for (int p = 0; p < n_points; p++) {
    const float* X = points + 3 * (size_t)p;
    float* o = points_out + 3 * (size_t)p;
    const int row = point_gba_row[p], r = ref[p];
    memcpy(o, X, 12);
    if (row >= 0) {
      if (row < n_gba_points) {
        memcpy(o, gba_points + 3 * (size_t)row, 12);
        result->n_taken++;
      } else {
        result->n_left++;
      }
    } else if (r >= 0 && r < n_kf && kf_out[r].status != ORBFE_GBA_MAP_KF_UNREACHED) {
      gm_move_point(poses + 12 * (size_t)r, kf_out[r].Twc, X, o);
      result->n_moved++;
    } else {
      result->n_left++;
    }
  }
}
