// mappoint_internal.h -- the reading of MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth, once, for the
// kernels (mappoint_kernels.hip) and for host code that wants the same bits (tests/cpp_mappoint/host_arith.cpp).  __host__ __device__
// inline functions, compiled with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   MapPoint::ComputeDistinctiveDescriptors   L/src/MapPoint.cc:229-320
//   MapPoint::UpdateNormalAndDepth            L/src/MapPoint.cc:340-381
//
// Descriptor.  live = the observations whose keyframe is not bad, in list order, N = |live|.  Row i = the N Hamming distances from
// live descriptor i to every live descriptor, its own 0 included (`Distances[i][i] = 0`); median_i = vDists[0.5 * (N - 1)] of the
// sorted row -- the index is a double truncated to size_t, the FLOOR of (N - 1) / 2; the winner is the first i with the least median
// (`median < BestMedian`, strict).  Consequences: for N = 1 the only row is {0}; for N = 2 both rows are {0, d} and index 0 picks the 0
// of each, so the first live observation always wins.  A distance is at most 256, which needs NINE bits: {a ^ 1, a, ~a, ~a} has the
// rows {0,1,255,255} {1,0,256,256} {255,256,0,0} {255,256,0,0} with medians 1, 1, 0, 0 and the winner 2; with the 256 kept in eight
// bits (0) row 1 becomes {0,0,0,1} and wins with median 0.
// The sorted row is never formed: the element of rank k of a row is the least value v with |{j : d_ij <= v}| >= k + 1, found by
// bisection over v in 0 .. 256 (nine rounds of a count, mp_select).  The winner is the least (median << 16) | i.
//
// Normal and depth, over ALL observations (isBad() is not read at :357-367): cv::Mat arithmetic as mapping_internal.h reads it --
// `mWorldPos - Owi` a float difference, cv::norm a double sum in element order and a double sqrt, `Mat / scalar` a product with
// (float)(1.0 / scalar), `normal + x` a float sum.  The sum runs sequentially in list order from 0.0f (a tree reduction gives other
// bytes).  tri_pair (mapping_internal.h) is this reading for two observations; the norm helpers are shared with it.
// An observation at zero distance from the point divides by zero as the reference does and follows IEEE (inf, then nan in the sum);
// that case is not covered by any test.
#pragma once
#include "mapping_internal.h"

#define MP_HD __host__ __device__ __forceinline__
#define MP_SMALL_OBS 64       // a point with at most this many observations is one wave's; a larger one a workgroup's
#define MP_SMALL_WAVES 4      // points per workgroup of the wave kernel
#define MP_LARGE_THREADS 256  // threads of the workgroup kernel
#define MP_DIST_NONE 0x1ffu   // what a column that is not live holds in the wave kernel: behind every distance

MP_HD int mp_median_index(int N) { return (int)(0.5 * (double)(N - 1)); }   // vDists[0.5 * (N - 1)]

// ORBmatcher::DescriptorDistance on eight dwords
MP_HD uint32_t mp_hamming(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) d += (uint32_t)__builtin_popcount(a[w] ^ b[w]);
  return d;
}

// the element of rank k (0-based) among dist(0) .. dist(n - 1), each in 0 .. 256: nine rounds, all of them always (a round with
// lo == hi changes nothing), so that every lane of a wave runs the same instructions
template <class Dist>
MP_HD uint32_t mp_select(int n, int k, Dist dist) {
  uint32_t lo = 0, hi = 256;
  for (int round = 0; round < 9; round++) {
    const uint32_t mid = (lo + hi) >> 1;
    int c = 0;
    for (int j = 0; j < n; j++) c += dist(j) <= mid ? 1 : 0;
    if (c >= k + 1) hi = mid; else lo = mid + 1;
  }
  return lo;
}

MP_HD uint32_t mp_key(uint32_t median, uint32_t i) { return (median << 16) | i; }   // least key = first row of the least median

// normali / cv::norm(normali) of one observation (:365-366)
MP_HD void mp_unit_term(const float* pos, const float* Ow, float* term) {
  const float d[3] = {pos[0] - Ow[0], pos[1] - Ow[1], pos[2] - Ow[2]};
  const float r = (float)(1.0 / tri_norm3(d));
  term[0] = d[0] * r; term[1] = d[1] * r; term[2] = d[2] * r;
}
MP_HD float mp_inv_count(int n) { return (float)(1.0 / (double)n); }   // normal / n
// :370-378
MP_HD void mp_depth_range(const float* pos, const float* Ow_ref, float sf_octave, float sf_top, float* min_distance, float* max_distance) {
  const float PC[3] = {pos[0] - Ow_ref[0], pos[1] - Ow_ref[1], pos[2] - Ow_ref[2]};
  const float dist = (float)tri_norm3(PC);
  *max_distance = dist * sf_octave;
  *min_distance = *max_distance / sf_top;
}

// what a point's own wave or workgroup checks before it reads anything else of the point
MP_HD bool mp_header_ok(const orbfe_mp_point& Q, int n_obs_total, int n_levels) {
  return Q.n_obs >= 0 && Q.n_obs <= ORBFE_MP_MAX_OBS && Q.obs_offset >= 0 && Q.obs_offset <= n_obs_total - Q.n_obs &&
         (Q.n_obs == 0 || (Q.ref >= 0 && Q.ref < Q.n_obs && Q.ref_octave >= 0 && Q.ref_octave < n_levels));
}
MP_HD bool mp_obs_kf_ok(const orbfe_mp_obs& o, int n_kf) { return o.kf >= 0 && o.kf < n_kf; }
// dwords: the descriptor block is read as dwords where it lies (the device form), so it has to be 4-byte aligned
MP_HD bool mp_obs_idx_ok(const orbfe_mp_obs& o, const orbfe_mp_keyframe& K, bool dwords) {
  return o.idx >= 0 && o.idx < K.n_keys && (!dwords || (K.desc & 3) == 0);
}

// The whole reading for one point, sequentially: what the two kernels spread over lanes.  desc_of(j) -> the eight dwords of
// observation j's descriptor.  Writes the halves `flags` selects and the status.
template <class DescOf>
MP_HD void mp_refresh_sequential(const orbfe_mp_point& Q, const orbfe_mp_obs* obs, const orbfe_mp_keyframe* kfs, int n_kf, int n_obs_total,
                                 const float* pos, const float* scale_factors, int n_levels, int flags, bool dwords, DescOf desc_of,
                                 orbfe_mp_update& U) {
  bool ok = mp_header_ok(Q, n_obs_total, n_levels);
  for (int j = 0; ok && j < Q.n_obs; j++) {
    const orbfe_mp_obs o = obs[Q.obs_offset + j];
    ok = mp_obs_kf_ok(o, n_kf) && mp_obs_idx_ok(o, kfs[o.kf], dwords);
  }
  U.status = !ok ? ORBFE_MP_REFUSED : Q.n_obs == 0 ? ORBFE_MP_UNCHANGED : ORBFE_MP_UPDATED;
  if (flags & ORBFE_MP_DESCRIPTOR) {
    U.best = -1;
    U.n_live = 0;
    for (int b = 0; b < 32; b++) U.desc[b] = 0;
  }
  if (flags & ORBFE_MP_NORMAL_DEPTH) U.normal[0] = U.normal[1] = U.normal[2] = U.min_distance = U.max_distance = 0.0f;
  if (U.status != ORBFE_MP_UPDATED) return;
  const orbfe_mp_obs* O = obs + Q.obs_offset;
  if (flags & ORBFE_MP_DESCRIPTOR) {
    int N = 0;
    for (int j = 0; j < Q.n_obs; j++) N += kfs[O[j].kf].bad ? 0 : 1;
    U.n_live = N;
    uint32_t best_key = 0xffffffffu;
    const int k = mp_median_index(N);
    for (int i = 0; i < Q.n_obs; i++) {
      if (kfs[O[i].kf].bad) continue;
      const uint32_t* di = desc_of(i);
      const uint32_t median = mp_select(Q.n_obs, k, [&](int j) { return kfs[O[j].kf].bad ? MP_DIST_NONE : mp_hamming(di, desc_of(j)); });
      const uint32_t key = mp_key(median, (uint32_t)i);
      if (key < best_key) best_key = key;
    }
    if (N > 0) {
      U.best = (int32_t)(best_key & 0xffffu);
      const uint32_t* d = desc_of(U.best);
      for (int b = 0; b < 32; b++) U.desc[b] = (uint8_t)(d[b >> 2] >> (8 * (b & 3)));
    }
  }
  if (flags & ORBFE_MP_NORMAL_DEPTH) {
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (int j = 0; j < Q.n_obs; j++) {
      float t[3];
      mp_unit_term(pos, kfs[O[j].kf].Ow, t);
      sum[0] = sum[0] + t[0]; sum[1] = sum[1] + t[1]; sum[2] = sum[2] + t[2];
    }
    const float inv_n = mp_inv_count(Q.n_obs);
    U.normal[0] = sum[0] * inv_n; U.normal[1] = sum[1] * inv_n; U.normal[2] = sum[2] * inv_n;
    mp_depth_range(pos, kfs[O[Q.ref].kf].Ow, scale_factors[Q.ref_octave], scale_factors[n_levels - 1], &U.min_distance, &U.max_distance);
  }
}

// ---- launcher (mappoint_kernels.hip)
struct MpLaunch {
  const orbfe_mp_keyframe* kfs; int n_kf;
  const orbfe_mp_obs* obs; int n_obs_total;
  const orbfe_mp_point* points; int P;
  const uint8_t* pos; int pos_stride;      // position of point p: three floats at pos + p * pos_stride
  const uint8_t* staged;                   // NULL: observation j's descriptor is kfs[kf].desc + idx * 32; else staged + j * 32, j its
                                           // row of the observation array (the host form)
  float scale_factors[ORBFE_MAX_LEVELS]; int n_levels;
  int flags;
  orbfe_mp_update* out;
};
void orbfe_launch_refresh_map_points(const MpLaunch& L, hipStream_t s);
