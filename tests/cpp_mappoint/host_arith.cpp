// host_arith.cpp -- csrc/mappoint_internal.h compiled for the HOST: the rank selection by counting, the winner key, the unit vectors
// and their ordered sum, the distance range and the checks that mappoint_kernels.hip spreads over lanes, so that the arithmetic the
// kernels execute can be compared with the yardstick on a machine without a GPU (tests/test_mappoint_cpu.py), and timed on one
// thread beside the kernels (tools/bench_map_points.py).  Same flags as the library (-ffp-contract=off).
#include <string.h>

#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/mappoint_internal.h"

extern "C" int mappoint_host_median_index(int N) { return mp_median_index(N); }
extern "C" int mappoint_host_small_obs(void) { return MP_SMALL_OBS; }

// the element of rank k of n values in 0 .. 256
extern "C" int mappoint_host_select(const int32_t* d, int n, int k) {
  return (int)mp_select(n, k, [d](int j) { return (uint32_t)d[j]; });
}

// P points as orbfe_refresh_map_points takes them (HOST addresses in the table), one after the other on the calling thread
extern "C" void mappoint_host_refresh(const orbfe_mp_keyframe* kfs, int n_kf, const orbfe_mp_obs* obs, int n_obs_total,
                                      const orbfe_mp_point* points, const float* positions, int P, const float* scale_factors, int n_levels,
                                      int flags, orbfe_mp_update* updates) {
  std::vector<uint32_t> rows;
  for (int p = 0; p < P; p++) {
    const orbfe_mp_point Q = points[p];
    // the point's descriptor rows as dwords, where its observations are in range (the reading checks them again)
    const bool header = mp_header_ok(Q, n_obs_total, n_levels);
    rows.assign(header ? (size_t)Q.n_obs * 8 : 0, 0u);
    for (int j = 0; header && j < Q.n_obs; j++) {
      const orbfe_mp_obs o = obs[Q.obs_offset + j];
      if (mp_obs_kf_ok(o, n_kf) && mp_obs_idx_ok(o, kfs[o.kf], false) && kfs[o.kf].desc)
        memcpy(&rows[(size_t)j * 8], reinterpret_cast<const uint8_t*>((uintptr_t)kfs[o.kf].desc) + (size_t)o.idx * 32, 32);
    }
    const uint32_t* base = rows.data();
    mp_refresh_sequential(Q, obs, kfs, n_kf, n_obs_total, positions + (size_t)3 * p, scale_factors, n_levels, flags, false,
                          [base](int j) { return base + (size_t)j * 8; }, updates[p]);
  }
}
