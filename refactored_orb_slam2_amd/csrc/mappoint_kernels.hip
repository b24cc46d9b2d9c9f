// mappoint_kernels.hip -- MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth for a ragged batch of points
// (include/orbfe.h: orbfe_refresh_map_points*).  The arithmetic is csrc/mappoint_internal.h's; this file spreads it over lanes.
//
// Two size classes, chosen per point by n_obs, one launch each over all P points (a point that belongs to the other class leaves at
// once; nothing crosses points, so a point's bytes do not depend on P or on its place):
//   mp_wave_kernel    n_obs <= 64: one wave per point, one observation per lane.  A lane keeps its descriptor in eight VGPRs; column j
//                     of the distance matrix is descriptor j read through v_readlane (scalar operands of the xor) and a popcount sum,
//                     kept in a VGPR of its own (a column that is not live holds MP_DIST_NONE), so a lane ends with its whole row in
//                     registers.  The row median is mp_select's bisection -- nine rounds of compare-and-count over the row --, the
//                     winner one wave minimum over (median << 16) | lane.  The unit vectors are formed one per lane and summed in
//                     list order through v_readlane.  It also writes the refusal of a point whose header is out of range.
//   mp_group_kernel   64 < n_obs <= 1024: one workgroup of 256 threads per point.  The live descriptors are compacted in list order
//                     into LDS once (32 B each; a prefix sum over the live flags gives the rank); wave w takes rows w, w + 4, ..: the
//                     row's descriptor is a broadcast LDS read, lane l forms columns l, l + 64, .. (at most 16) into registers, and a
//                     round of mp_select's bisection is one compare and one ballot per 64 columns with lo, hi and the count in
//                     SGPRs: no N x N matrix exists anywhere.  The unit vectors go to LDS and three threads add one component
//                     each in list order.
// Every index is checked before it is used; no floating-point atomics; no scratch memory (arrays are indexed by unrolled constants).
#include "mappoint_internal.h"

static_assert(sizeof(orbfe_mp_keyframe) == 32 && sizeof(orbfe_mp_obs) == 8 && sizeof(orbfe_mp_point) == 16 && sizeof(orbfe_mp_update) == 64,
              "record layout");
static_assert(MP_SMALL_OBS == 64, "one observation per lane");
static_assert(ORBFE_MP_MAX_OBS == 4 * MP_LARGE_THREADS, "four consecutive observations per thread in the validation pass");

namespace {

__device__ __forceinline__ uint32_t lane_u32(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ float lane_f32(float v, int lane) { return __uint_as_float(lane_u32(__float_as_uint(v), lane)); }

// scale_factors[level] of the by-value launch record without an indexed read of it (which would put the record in scratch memory)
__device__ __forceinline__ float pick_level(const MpLaunch& L, int level) {
  float v = 0.0f;
#pragma unroll
  for (int l = 0; l < ORBFE_MAX_LEVELS; l++) v = l == level ? L.scale_factors[l] : v;
  return v;
}

__device__ __forceinline__ const float* position_of(const MpLaunch& L, int p) {
  return reinterpret_cast<const float*>(L.pos + (size_t)p * (size_t)L.pos_stride);
}
// observation j (row g of the observation array) of a checked point: its eight dwords
__device__ __forceinline__ const uint32_t* descriptor_of(const MpLaunch& L, int g, const orbfe_mp_obs& o, const orbfe_mp_keyframe& K) {
  return reinterpret_cast<const uint32_t*>(L.staged ? L.staged + (size_t)g * 32 : reinterpret_cast<const uint8_t*>(K.desc) + (size_t)o.idx * 32);
}

// status and the selected halves of a point that is refused or unchanged; `t` = a thread index of the point's wave or workgroup
__device__ __forceinline__ void write_nothing(const MpLaunch& L, orbfe_mp_update* U, int status, int t) {
  if (t == 0) {
    U->status = status;
    if (L.flags & ORBFE_MP_DESCRIPTOR) {
      U->best = -1;
      U->n_live = 0;
    }
    if (L.flags & ORBFE_MP_NORMAL_DEPTH) {
      U->normal[0] = U->normal[1] = U->normal[2] = 0.0f;
      U->min_distance = U->max_distance = 0.0f;
    }
  }
  if ((L.flags & ORBFE_MP_DESCRIPTOR) && t < 8) reinterpret_cast<uint32_t*>(U->desc)[t] = 0u;
}

__global__ __launch_bounds__(MP_SMALL_WAVES * 64) void mp_wave_kernel(const MpLaunch L) {
  const int lane = threadIdx.x & 63;
  const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * MP_SMALL_WAVES + (threadIdx.x >> 6)));
  if (p >= L.P) return;
  const orbfe_mp_point Q = L.points[p];
  const bool header = mp_header_ok(Q, L.n_obs_total, L.n_levels);
  if (header && Q.n_obs > MP_SMALL_OBS) return;   // mp_group_kernel's
  orbfe_mp_update* U = L.out + p;
  const int n = __builtin_amdgcn_readfirstlane(header ? Q.n_obs : 0);

  bool bad_obs = false, live = false;
  float Ow[3] = {0.0f, 0.0f, 0.0f};
  const uint32_t* dp = nullptr;
  if (lane < n) {
    const int g = Q.obs_offset + lane;
    const orbfe_mp_obs o = L.obs[g];
    bad_obs = !mp_obs_kf_ok(o, L.n_kf);
    if (!bad_obs) {
      const orbfe_mp_keyframe K = L.kfs[o.kf];
      bad_obs = !mp_obs_idx_ok(o, K, L.staged == nullptr);
      if (!bad_obs) {
        live = K.bad == 0;
        Ow[0] = K.Ow[0]; Ow[1] = K.Ow[1]; Ow[2] = K.Ow[2];
        dp = descriptor_of(L, g, o, K);
      }
    }
  }
  const bool refused = !header || __ballot(bad_obs) != 0ull;
  if (refused || n == 0) {
    write_nothing(L, U, refused ? ORBFE_MP_REFUSED : ORBFE_MP_UNCHANGED, lane);
    return;
  }
  if (lane == 0) U->status = ORBFE_MP_UPDATED;

  if (L.flags & ORBFE_MP_DESCRIPTOR) {
    const uint64_t live_mask = __ballot(live);
    const int N = __popcll(live_mask);
    uint32_t d[8];
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = live ? dp[w] : 0u;
    // the lane's row, one register per column
    uint32_t dist[MP_SMALL_OBS];
#pragma unroll
    for (int j = 0; j < MP_SMALL_OBS; j++) {
      dist[j] = MP_DIST_NONE;
      if (j < n) {   // wave-uniform
        uint32_t b[8];
#pragma unroll
        for (int w = 0; w < 8; w++) b[w] = lane_u32(d[w], j);
        const uint32_t h = mp_hamming(d, b);
        dist[j] = (live_mask >> j) & 1ull ? h : MP_DIST_NONE;
      }
    }
    // mp_select over the registers: columns that are not live never count (MP_DIST_NONE > 256)
    const int k = mp_median_index(N);
    uint32_t lo = 0, hi = 256;
#pragma unroll 1
    for (int round = 0; round < 9; round++) {
      const uint32_t mid = (lo + hi) >> 1;
      int c = 0;
#pragma unroll
      for (int j0 = 0; j0 < MP_SMALL_OBS; j0 += 8) {
        if (j0 < n) {   // wave-uniform
#pragma unroll
          for (int j = j0; j < j0 + 8; j++) c += dist[j] <= mid ? 1 : 0;
        }
      }
      if (c >= k + 1) hi = mid; else lo = mid + 1;
    }
    uint32_t key = live ? mp_key(lo, (uint32_t)lane) : 0xffffffffu;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)key, off);
      key = other < key ? other : key;
    }
    const int best = N > 0 ? (int)(key & 0xffffu) : -1;
    if (lane == 0) {
      U->best = best;
      U->n_live = N;
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(U->desc);
    if (N == 0) {
      if (lane < 8) out[lane] = 0u;
    } else if (lane == best) {
#pragma unroll
      for (int w = 0; w < 8; w++) out[w] = d[w];
    }
  }

  if (L.flags & ORBFE_MP_NORMAL_DEPTH) {
    const float* X = position_of(L, p);
    const float pos[3] = {X[0], X[1], X[2]};
    float t[3] = {0.0f, 0.0f, 0.0f};
    if (lane < n) mp_unit_term(pos, Ow, t);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int j = 0; j < n; j++) {   // list order; every lane forms the same sum
      sx = sx + lane_f32(t[0], j);
      sy = sy + lane_f32(t[1], j);
      sz = sz + lane_f32(t[2], j);
    }
    const int ref = __builtin_amdgcn_readfirstlane(Q.ref);
    const float Or[3] = {lane_f32(Ow[0], ref), lane_f32(Ow[1], ref), lane_f32(Ow[2], ref)};
    if (lane == 0) {
      const float inv_n = mp_inv_count(n);
      U->normal[0] = sx * inv_n; U->normal[1] = sy * inv_n; U->normal[2] = sz * inv_n;
      float mn, mx;
      mp_depth_range(pos, Or, pick_level(L, Q.ref_octave), pick_level(L, L.n_levels - 1), &mn, &mx);
      U->min_distance = mn;
      U->max_distance = mx;
    }
  }
}

__global__ __launch_bounds__(MP_LARGE_THREADS) void mp_group_kernel(const MpLaunch L) {
  __shared__ __attribute__((aligned(16))) uint32_t s_desc[ORBFE_MP_MAX_OBS * 8];   // live descriptors by rank
  __shared__ float s_term[3][ORBFE_MP_MAX_OBS];                                   // unit vectors by list position
  __shared__ uint16_t s_pos[ORBFE_MP_MAX_OBS];                                    // list position of a rank
  __shared__ int s_count[MP_LARGE_THREADS / 64];
  __shared__ uint32_t s_key[MP_LARGE_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const orbfe_mp_point Q = L.points[p];
  if (!mp_header_ok(Q, L.n_obs_total, L.n_levels) || Q.n_obs <= MP_SMALL_OBS) return;   // mp_wave_kernel's, a bad header included
  orbfe_mp_update* U = L.out + p;
  const int n = Q.n_obs;
  const float* X = position_of(L, p);
  const float pos[3] = {X[0], X[1], X[2]};

  // observations 4 tid .. 4 tid + 3: the checks, the live flags, the unit vectors
  bool bad_obs = false;
  uint32_t live_bits = 0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int j = 4 * tid + c;
    if (j >= n) continue;
    const orbfe_mp_obs o = L.obs[Q.obs_offset + j];
    if (!mp_obs_kf_ok(o, L.n_kf)) {
      bad_obs = true;
      continue;
    }
    const orbfe_mp_keyframe K = L.kfs[o.kf];
    if (!mp_obs_idx_ok(o, K, L.staged == nullptr)) {
      bad_obs = true;
      continue;
    }
    if (K.bad == 0) live_bits |= 1u << c;
    if (L.flags & ORBFE_MP_NORMAL_DEPTH) {
      float t[3];
      mp_unit_term(pos, K.Ow, t);
      s_term[0][j] = t[0]; s_term[1][j] = t[1]; s_term[2][j] = t[2];
    }
  }
  if (__syncthreads_or(bad_obs ? 1 : 0)) {
    write_nothing(L, U, ORBFE_MP_REFUSED, tid);
    return;
  }
  if (tid == 0) U->status = ORBFE_MP_UPDATED;

  if (L.flags & ORBFE_MP_NORMAL_DEPTH) {   // the last wave has the fewest rows below
    const int t = tid - (MP_LARGE_THREADS - 64);
    if (t >= 0 && t < 3) {
      float sum = 0.0f;
      for (int j = 0; j < n; j++) sum = sum + s_term[t][j];   // list order
      U->normal[t] = sum * mp_inv_count(n);
    } else if (t == 3) {
      const orbfe_mp_obs o = L.obs[Q.obs_offset + Q.ref];   // checked above
      const orbfe_mp_keyframe K = L.kfs[o.kf];
      float mn, mx;
      mp_depth_range(pos, K.Ow, pick_level(L, Q.ref_octave), pick_level(L, L.n_levels - 1), &mn, &mx);
      U->min_distance = mn;
      U->max_distance = mx;
    }
  }
  if (!(L.flags & ORBFE_MP_DESCRIPTOR)) return;

  // rank of every live observation: prefix sum over the per-thread counts
  const int cnt = __popc(live_bits);
  int incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  if (lane == 63) s_count[wave] = incl;
  __syncthreads();
  int base = 0, N = 0;
#pragma unroll
  for (int w = 0; w < MP_LARGE_THREADS / 64; w++) {
    base += w < wave ? s_count[w] : 0;
    N += s_count[w];
  }
  N = __builtin_amdgcn_readfirstlane(N);   // the same in every lane: say so
  int rank = base + incl - cnt;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (!((live_bits >> c) & 1u)) continue;
    const int j = 4 * tid + c;
    const orbfe_mp_obs o = L.obs[Q.obs_offset + j];
    const orbfe_mp_keyframe K = L.kfs[o.kf];
    const uint32_t* dp = descriptor_of(L, Q.obs_offset + j, o, K);
#pragma unroll
    for (int w = 0; w < 8; w++) s_desc[rank * 8 + w] = dp[w];
    s_pos[rank] = (uint16_t)j;
    rank++;
  }
  __syncthreads();

  // one row per wave at a time: lane l holds columns l, l + 64, .. of the row in registers (a column behind N holds MP_DIST_NONE), so a
  // round of mp_select's bisection is one compare and one ballot per 64 columns, and lo, hi and the count are scalars
  const int k = mp_median_index(N);
  uint32_t key = 0xffffffffu;
  for (int i = __builtin_amdgcn_readfirstlane(wave); i < N; i += MP_LARGE_THREADS / 64) {
    uint32_t a[8];
#pragma unroll
    for (int w = 0; w < 8; w++) a[w] = s_desc[i * 8 + w];
    uint32_t dist[ORBFE_MP_MAX_OBS / 64];
#pragma unroll
    for (int c = 0; c < ORBFE_MP_MAX_OBS / 64; c++) {
      dist[c] = MP_DIST_NONE;
      if (c * 64 < N) {   // wave-uniform
        const int j = c * 64 + lane;
        if (j < N) dist[c] = mp_hamming(a, &s_desc[j * 8]);
      }
    }
    uint32_t lo = 0, hi = 256;
#pragma unroll 1
    for (int round = 0; round < 9; round++) {
      const uint32_t mid = (lo + hi) >> 1;
      int cnt = 0;
#pragma unroll
      for (int c = 0; c < ORBFE_MP_MAX_OBS / 64; c++)
        if (c * 64 < N) cnt += __popcll(__ballot(dist[c] <= mid));
      if (cnt >= k + 1) hi = mid; else lo = mid + 1;
    }
    const uint32_t mine = mp_key(lo, (uint32_t)i);
    key = mine < key ? mine : key;
  }
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < MP_LARGE_THREADS / 64; w++) key = s_key[w] < key ? s_key[w] : key;
  uint32_t* out = reinterpret_cast<uint32_t*>(U->desc);
  if (N == 0) {
    if (tid == 0) {
      U->best = -1;
      U->n_live = 0;
    }
    if (tid < 8) out[tid] = 0u;
    return;
  }
  const int best_rank = (int)(key & 0xffffu);
  if (tid == 0) {
    U->best = (int)s_pos[best_rank];
    U->n_live = N;
  }
  if (tid < 8) out[tid] = s_desc[best_rank * 8 + tid];
}

}  // namespace

void orbfe_launch_refresh_map_points(const MpLaunch& L, hipStream_t s) {
  if (L.P <= 0) return;
  hipLaunchKernelGGL(mp_wave_kernel, dim3((unsigned)((L.P + MP_SMALL_WAVES - 1) / MP_SMALL_WAVES)), dim3(MP_SMALL_WAVES * 64), 0, s, L);
  hipLaunchKernelGGL(mp_group_kernel, dim3((unsigned)L.P), dim3(MP_LARGE_THREADS), 0, s, L);
}
