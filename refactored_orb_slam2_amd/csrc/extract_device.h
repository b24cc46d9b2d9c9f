// extract_device.h -- what more than one of the extractor's kernel units (pyramid_kernels.hip, fast_kernels.hip, octree_kernels.hip,
// describe_kernels.hip) uses: the wave size, the wave and block scans, and the -DFC_TIMING=1 phase clock.  Device code only.
#pragma once

#define WAVE 64

// -DFC_TIMING=1 instrumentation (tools/fc_phase_profile.py, step_phase_profile.py, oct_phase_profile.py): every unit keeps its
// profile array and its orbfe_debug_*_profile function beside its kernel.  FC_T(i) adds the cycles since the last call to the
// kernel's accumulator tacc<i>.
#ifndef FC_TIMING
#define FC_TIMING 0
#endif
#if FC_TIMING
#define FC_T(i) do { const uint32_t _t = (uint32_t)__builtin_readcyclecounter(); tacc##i += _t - tprev; tprev = _t; } while (0)
#else
#define FC_T(i)
#endif

__device__ __forceinline__ int wave_incl_scan(int v) {
  // DPP row shifts + row broadcasts (gfx9): six VALU adds, no LDS crossbar round trips (ds_bpermute) as with __shfl_up
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
  return v;
}

// Inclusive scan over the T threads of a block (thread order = threadIdx.x; T a multiple of 64, <= 1024).  tmp: >= 16 ints of LDS.
// Returns the inclusive prefix; *total receives the block sum.  Contains two __syncthreads().
template <int T>
__device__ __forceinline__ int block_incl_scan_t(int v, int* tmp, int* total) {
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid >> 6;
  int s = wave_incl_scan(v);
  if (T == WAVE) {   // one wave: no LDS, no barrier
    *total = __builtin_amdgcn_readlane(s, WAVE - 1);
    return s;
  }
  __syncthreads();  // protect tmp from a previous use
  if (lane == WAVE - 1) tmp[wid] = s;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < T / WAVE; i++) {
    int t = tmp[i];
    if (i < wid) off += t;
    tot += t;
  }
  *total = tot;
  return s + off;
}

// The same with ONE barrier: consecutive calls alternate between two slots of `tmp` (2 * T / WAVE ints, used by nothing else), so a
// call's writes cannot meet the reads of the call before it -- those lie in front of this call's predecessor's barrier.
template <int T>
__device__ __forceinline__ int block_incl_scan_alt(int v, int* tmp, int& slot, int* total) {
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid >> 6;
  const int s = wave_incl_scan(v);
  int* t = tmp + slot * (T / WAVE);
  slot ^= 1;
  if (lane == WAVE - 1) t[wid] = s;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < T / WAVE; i++) {
    const int x = t[i];
    if (i < wid) off += x;
    tot += x;
  }
  *total = tot;
  return s + off;
}
