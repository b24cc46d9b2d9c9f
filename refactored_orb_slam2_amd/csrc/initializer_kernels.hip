// initializer_kernels.hip -- Initializer::Initialize (L/src/Initializer.cc:45-122) for P problems in five launches without a host
// round trip.  The arithmetic is initializer_internal.h; this file stages, distributes, reduces and scans.
//   initz_prologue_kernel    one workgroup per problem: the match list (i, matches12[i] >= 0) compacted in index order by ballots of
//     one wave, both key lists staged in LDS and Normalize's four float sums (x and y of two frames) each in index order on a lane of
//     its own, T1, T2inv, T2t.
//   initz_hypotheses_kernel  grid (ceil(h_cap / INI_WAVES), 2 models, P): a workgroup stages the problem's matches in LDS (16 bytes
//     each), then each wave takes one hypothesis of one model.  The 9-column decomposition is spread over the wave -- a lane holds one
//     row of [A; V] in nine named doubles, the 36 pairs of a sweep are unrolled, the column dot products are 16-lane butterflies --
//     the model behind it is wave-uniform and moved into SGPRs, and the wave scores all N matches 64 at a time: a ballot IS the
//     inlier word, a lane's score terms are added in match order and the 64 lane sums in one butterfly, an order that depends on N
//     only.
//   initz_select_kernel      one wave per problem: the first maximum per model, RH and the model, then DecomposeE's four or Faugeras'
//     eight motions on named scalars; copies the chosen model's inlier words.
//   initz_checkrt_kernel     one workgroup per (problem, candidate): triangulates the inliers, counts the good ones, keeps their
//     cosines as ordered keys in LDS and takes the order statistic min(50, nGood - 1) by exact rank counting.
//   initz_decide_kernel      one workgroup per problem: the acceptance rules; on success the winner's points are computed once more
//     (the same function, the same bits) and scattered to P3D and the triangulated words.
// No float atomics, no scratch; a hypothesis' bytes depend on its problem and its set only.
#include "initializer_internal.h"

#define INI_THREADS (INI_WAVES * 64)
static_assert(sizeof(orbfe_init_params) == 32 && sizeof(orbfe_init_hypothesis) == 64 && sizeof(orbfe_init_candidate) == 64 &&
              sizeof(orbfe_init_result) == 224 && sizeof(IniHeader) == 160, "record layout");

__device__ __forceinline__ int ini_clamp(int v, int cap) { return min(max(v, 0), cap); }
__device__ __forceinline__ float ini_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

__global__ __launch_bounds__(256) void initz_prologue_kernel(IniLaunch L) {
  extern __shared__ float sk[];   // [2][cap][2]
  const int p = blockIdx.x, tid = threadIdx.x, cap = L.cap;
  const int n1 = ini_clamp(L.n1[p], cap), n2 = ini_clamp(L.n2[p], cap);
  const float* keys1 = L.keys1 + (size_t)p * cap * 2;
  const float* keys2 = L.keys2 + (size_t)p * cap * 2;
  for (int i = tid; i < 2 * n1; i += 256) sk[i] = keys1[i];
  for (int i = tid; i < 2 * n2; i += 256) sk[2 * cap + i] = keys2[i];
  __syncthreads();
  if (tid >= 64) return;
  const int lane = tid;
  const int32_t* m12 = L.matches12 + (size_t)p * cap;
  float4* mxy = L.mxy + (size_t)p * cap;
  int32_t* mi1 = L.mi1 + (size_t)p * cap;
  int N = 0;
  for (int base = 0; base < n1; base += 64) {
    const int i = base + lane;
    const int m = i < n1 ? m12[i] : -1;
    const bool ok = m >= 0 && m < n2;
    const uint64_t b = __ballot(ok);
    if (ok) {
      const int pos = N + __popcll(b & ((1ull << lane) - 1ull));
      mxy[pos] = make_float4(sk[2 * i], sk[2 * i + 1], sk[2 * cap + 2 * m], sk[2 * cap + 2 * m + 1]);
      mi1[pos] = i;
    }
    N += __popcll(b);
  }
  // lane 0: x of frame 1, lane 1: y of frame 1, lane 2: x of frame 2, lane 3: y of frame 2
  float mean = 0.0f, scale = 0.0f;
  if (lane < 4) ini_normalize_coordinate(sk + (lane >> 1) * 2 * cap + (lane & 1), 2, (lane >> 1) ? n2 : n1, mean, scale);
  IniNorm N1, N2;
  N1.mx = __shfl(mean, 0); N1.my = __shfl(mean, 1); N1.sx = __shfl(scale, 0); N1.sy = __shfl(scale, 1);
  N2.mx = __shfl(mean, 2); N2.my = __shfl(mean, 3); N2.sx = __shfl(scale, 2); N2.sy = __shfl(scale, 3);
  if (lane == 0) {
    IniHeader h;
    h.N = N; h.n1 = n1; h.n2 = n2; h.pad = 0; h.pad2 = 0;
    h.N1 = N1; h.N2 = N2;
    float T2[9];
    ini_norm_matrix(N1, h.T1);
    ini_norm_matrix(N2, T2);
    ini_inv33(T2, h.T2inv);
    ini_transpose33(T2, h.T2t);
    L.header[p] = h;
  }
}

__global__ __launch_bounds__(INI_THREADS) void initz_hypotheses_kernel(IniLaunch L) {
  extern __shared__ float4 sm[];   // [N]
  const int p = blockIdx.z, model = blockIdx.y, cap = L.cap;
  const IniHeader& hd = L.header[p];
  const int N = hd.N, H = ini_clamp(L.H[p], L.h_cap);
  if (N < 8 || (int)blockIdx.x * INI_WAVES >= H) return;   // uniform
  for (int i = threadIdx.x; i < N; i += INI_THREADS) sm[i] = L.mxy[(size_t)p * cap + i];
  __syncthreads();
  const int h = (int)blockIdx.x * INI_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (h >= H) return;
  const size_t row = ((size_t)p * 2 + model) * L.h_cap + h;
  const int W = (cap + 63) >> 6, n_words = (N + 63) >> 6;
  uint64_t* words = L.words + row * W;
  uint32_t* rec = reinterpret_cast<uint32_t*>(L.hyps + row);
  const int32_t* set = L.sets + ((size_t)p * L.h_cap + h) * 8;
  const int32_t s8[8] = {set[0], set[1], set[2], set[3], set[4], set[5], set[6], set[7]};
  if (!ini_set_ok(s8, N)) {   // not a draw of :80-93: an all-zero record, nothing outside the problem is read
    for (int w = lane; w < n_words; w += 64) words[w] = 0;
    if (lane < 16) rec[lane] = 0u;
    return;
  }
  const IniNorm N1 = hd.N1, N2 = hd.N2;
  IniRow r = ini_row_v(lane - 16);
  if (lane < (model == 0 ? 16 : 8)) {
    const float4 m = sm[set[model == 0 ? lane >> 1 : lane]];   // the lane's own index: nothing is indexed in registers
    const float u1 = ini_norm_x(N1, m.x), v1 = ini_norm_y(N1, m.y), u2 = ini_norm_x(N2, m.z), v2 = ini_norm_y(N2, m.w);
    r = model == 0 ? ini_row_h(lane & 1, u1, v1, u2, v2) : ini_row_f(u1, v1, u2, v2);
  }
  float v9[9], M[9], Minv[9];
  ini_null9_wave(r, lane, v9);
  if (model == 0) {
    ini_model_h(v9, hd.T1, hd.T2inv, M, Minv);
  } else {
    ini_model_f(v9, hd.T1, hd.T2t, M);
#pragma unroll
    for (int k = 0; k < 9; k++) Minv[k] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < 9; k++) {
    M[k] = ini_uniform(M[k]);
    Minv[k] = ini_uniform(Minv[k]);
  }
  const float invSigmaSquare = ini_inv_sigma_square(L.params[p].sigma);
  float sc = 0.0f;
  int count = 0;
  for (int w = 0; w < n_words; w++) {
    const int i = w * 64 + lane;
    bool ok = false;
    float a1 = 0.0f, a2 = 0.0f;
    if (i < N) {
      const float4 m = sm[i];
      ok = model == 0 ? ini_check_h(M, Minv, m.x, m.y, m.z, m.w, invSigmaSquare, a1, a2) : ini_check_f(M, m.x, m.y, m.z, m.w, invSigmaSquare, a1, a2);
    }
    sc += a1;
    sc += a2;
    const uint64_t b = __ballot(ok);   // lanes behind N vote 0: the tail bits of the last word are zero
    if (lane == 0) words[w] = b;
    count += __popcll(b);
  }
  for (int d = 32; d > 0; d >>= 1) sc += __shfl_xor(sc, d);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) rec[k] = __float_as_uint(M[k]);
    rec[9] = __float_as_uint(sc);
    rec[10] = (uint32_t)count;
    rec[11] = 1u;
    rec[12] = 0u; rec[13] = 0u; rec[14] = 0u; rec[15] = 0u;
  }
}

// the first maximum over a model's H records: a lane scans its own in order, the lanes are merged by the order-free rule
__device__ __forceinline__ void ini_scan_best(const orbfe_init_hypothesis* hyps, int H, int lane, float& best_score, int& best) {
  best_score = 0.0f;
  best = -1;
  for (int h = lane; h < H; h += 64) ini_first_max(hyps[h].score, h, best_score, best);
  for (int d = 32; d > 0; d >>= 1) {
    const float os = __shfl_xor(best_score, d);
    const int ob = __shfl_xor(best, d);
    if (ob >= 0 && (best < 0 || os > best_score || (os == best_score && ob < best))) {
      best_score = os;
      best = ob;
    }
  }
}

__global__ __launch_bounds__(64) void initz_select_kernel(IniLaunch L) {
  const int p = blockIdx.x, lane = threadIdx.x, cap = L.cap;
  const IniHeader& hd = L.header[p];
  const int N = hd.N, n1 = hd.n1, H = N < 8 ? 0 : ini_clamp(L.H[p], L.h_cap);
  const int W = (cap + 63) >> 6, n1_words = (n1 + 63) >> 6;
  const orbfe_init_hypothesis* hyps_h = L.hyps + (size_t)p * 2 * L.h_cap;
  const orbfe_init_hypothesis* hyps_f = hyps_h + L.h_cap;
  float SH, SF;
  int bh, bf;
  ini_scan_best(hyps_h, H, lane, SH, bh);
  ini_scan_best(hyps_f, H, lane, SF, bf);
  const float RH = SH / (SH + SF);   // :110
  int model = 0;
  if (bh >= 0 || bf >= 0) model = (double)RH > 0.40 ? 1 : 2;   // :114
  orbfe_init_candidate* cands = L.cands + (size_t)p * 8;
  if (lane < 8) {
    uint32_t* cw = reinterpret_cast<uint32_t*>(cands + lane);
#pragma unroll
    for (int k = 0; k < 16; k++) cw[k] = 0u;
  }
  __syncthreads();
  if (lane == 0) {
    orbfe_init_result r;
    uint32_t* rw = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(orbfe_init_result) / 4); k++) rw[k] = 0u;
    r.best_h = bh; r.best_f = bf; r.score_h = SH; r.score_f = SF;
    r.rh = model ? RH : 0.0f;
    r.n_matches = N;
    r.model = model;
    r.best_candidate = -1;
    if (N >= 8) {   // below, the host form launches nothing and reports zeros
      r.norm1[0] = hd.N1.mx; r.norm1[1] = hd.N1.my; r.norm1[2] = hd.N1.sx; r.norm1[3] = hd.N1.sy;
      r.norm2[0] = hd.N2.mx; r.norm2[1] = hd.N2.my; r.norm2[2] = hd.N2.sx; r.norm2[3] = hd.N2.sy;
    }
    if (N < 8) r.reason = ORBFE_INIT_FEW_MATCHES;
    else if (!model) r.reason = ORBFE_INIT_NO_MODEL;
    float K[9];
    ini_K(L.params[p], K);
    if (bh >= 0) {
#pragma unroll
      for (int k = 0; k < 9; k++) r.H21[k] = hyps_h[bh].M[k];
    }
    if (bf >= 0) {
#pragma unroll
      for (int k = 0; k < 9; k++) r.F21[k] = hyps_f[bf].M[k];
    }
    if (model == 1) {
      r.n_inliers = hyps_h[bh].n_inliers;
      if (ini_candidates_h(r.H21, K, cands)) r.n_candidates = 8;
      else r.reason = ORBFE_INIT_H_DEGENERATE;
    } else if (model == 2) {
      r.n_inliers = hyps_f[bf].n_inliers;
      ini_candidates_f(r.F21, K, cands);
      r.n_candidates = 4;
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(L.result + p);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(orbfe_init_result) / 4); k++) out[k] = rw[k];
  }
  const int n_words = (N + 63) >> 6;
  const uint64_t* src = L.words + (((size_t)p * 2 + (model == 2 ? 1 : 0)) * L.h_cap + (model == 1 ? bh : (model == 2 ? bf : 0))) * W;
  for (int w = lane; w < n1_words; w += 64) L.inlier_words[(size_t)p * W + w] = (model && w < n_words) ? src[w] : 0;
}

__global__ __launch_bounds__(INI_RT_THREADS) void initz_checkrt_kernel(IniLaunch L) {
  __shared__ uint32_t keys[ORBFE_INIT_MAX_MATCHES];
  __shared__ int counts[INI_RT_THREADS];
  const int p = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, cap = L.cap;
  const orbfe_init_result& res = L.result[p];
  if (c >= res.n_candidates) return;   // uniform
  const int N = res.n_matches, W = (cap + 63) >> 6;
  const orbfe_init_params C = L.params[p];
  orbfe_init_candidate* cand = L.cands + (size_t)p * 8 + c;
  float K[9];
  ini_K(C, K);
  IniPose P;
  ini_pose(K, cand->R, cand->t, P);
  const float th2 = ini_th2(C.sigma);
  const uint64_t* inl = L.inlier_words + (size_t)p * W;
  const float4* mxy = L.mxy + (size_t)p * cap;
  int mine = 0;
  for (int i = tid; i < N; i += INI_RT_THREADS) {
    uint32_t key = 0xffffffffu;   // not a good point
    if ((inl[i >> 6] >> (i & 63)) & 1ull) {
      const float4 m = mxy[i];
      float x[3], cosv;
      if (ini_check_point(C, K, P, th2, m.x, m.y, m.z, m.w, x, cosv)) {
        key = ini_cos_key(cosv);
        mine++;
      }
    }
    keys[i] = key;
  }
  counts[tid] = mine;
  __syncthreads();
  for (int d = INI_RT_THREADS / 2; d > 0; d >>= 1) {
    if (tid < d) counts[tid] += counts[tid + d];
    __syncthreads();
  }
  const int nGood = counts[0];
  if (nGood == 0) {   // :896
    if (tid == 0) { cand->n_good = 0; cand->parallax = 0.0f; }
    return;
  }
  // :891-894: the element of rank min(50, size - 1) of the sorted cosines; the rank of a key is the number of keys below it, equal
  // keys in index order, so exactly one thread finds its rank equal to idx
  const int idx = min(50, nGood - 1);
  for (int i = tid; i < N; i += INI_RT_THREADS) {
    const uint32_t k = keys[i];
    if (k == 0xffffffffu) continue;
    int rank = 0;
    for (int j = 0; j < N; j++) {
      const uint32_t o = keys[j];
      rank += (o < k || (o == k && j < i)) ? 1 : 0;
    }
    if (rank == idx) {
      cand->n_good = nGood;
      cand->parallax = ini_parallax_degrees(ini_key_cos(k));
    }
  }
}

__global__ __launch_bounds__(INI_RT_THREADS) void initz_decide_kernel(IniLaunch L) {
  __shared__ int counts[INI_RT_THREADS];
  const int p = blockIdx.x, tid = threadIdx.x, cap = L.cap;
  const int W = (cap + 63) >> 6;
  const IniHeader& hd = L.header[p];
  const int n1 = hd.n1, n1_words = (n1 + 63) >> 6;
  float* P3D = L.P3D + (size_t)p * cap * 3;
  unsigned long long* tri = reinterpret_cast<unsigned long long*>(L.triangulated + (size_t)p * W);
  for (int i = tid; i < 3 * n1; i += INI_RT_THREADS) P3D[i] = 0.0f;
  for (int w = tid; w < n1_words; w += INI_RT_THREADS) tri[w] = 0ull;
  orbfe_init_result r = L.result[p];
  const orbfe_init_params C = L.params[p];
  const orbfe_init_candidate* cands = L.cands + (size_t)p * 8;
  bool success = false;
  if (r.n_candidates == 8) success = ini_decide_h(cands, r.n_inliers, C, r);
  else if (r.n_candidates == 4) success = ini_decide_f(cands, r.n_inliers, C, r);
  __syncthreads();
  int mine = 0;
  if (success) {   // uniform
    const orbfe_init_candidate* cand = cands + r.best_candidate;
    float K[9];
    ini_K(C, K);
    IniPose P;
    ini_pose(K, cand->R, cand->t, P);
    const float th2 = ini_th2(C.sigma);
    const uint64_t* inl = L.inlier_words + (size_t)p * W;
    const float4* mxy = L.mxy + (size_t)p * cap;
    const int32_t* mi1 = L.mi1 + (size_t)p * cap;
    const int N = r.n_matches;
    for (int i = tid; i < N; i += INI_RT_THREADS) {
      if (!((inl[i >> 6] >> (i & 63)) & 1ull)) continue;
      const float4 m = mxy[i];
      float x[3], cosv;
      const int code = ini_check_point(C, K, P, th2, m.x, m.y, m.z, m.w, x, cosv);
      if (!code) continue;
      const int i1 = mi1[i];
      P3D[3 * i1] = x[0]; P3D[3 * i1 + 1] = x[1]; P3D[3 * i1 + 2] = x[2];
      if (code == 2) {
        atomicOr(tri + (i1 >> 6), 1ull << (i1 & 63));   // an integer OR: the order does not show
        mine++;
      }
    }
  }
  counts[tid] = mine;
  __syncthreads();
  for (int d = INI_RT_THREADS / 2; d > 0; d >>= 1) {
    if (tid < d) counts[tid] += counts[tid + d];
    __syncthreads();
  }
  if (tid == 0) {
    r.success = success ? 1 : 0;
    r.n_triangulated = counts[0];
    if (success) {
      const orbfe_init_candidate* cand = cands + r.best_candidate;
#pragma unroll
      for (int k = 0; k < 9; k++) r.R21[k] = cand->R[k];
#pragma unroll
      for (int k = 0; k < 3; k++) r.t21[k] = cand->t[k];
    }
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(&r);
    uint32_t* out = reinterpret_cast<uint32_t*>(L.result + p);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(orbfe_init_result) / 4); k++) out[k] = rw[k];
  }
}

void orbfe_launch_initializer(const IniLaunch& L, int P, hipStream_t s) {
  if (P < 1 || L.cap < 1 || L.h_cap < 1) return;
  hipLaunchKernelGGL(initz_prologue_kernel, dim3(P), dim3(256), (size_t)L.cap * 16, s, L);
  hipLaunchKernelGGL(initz_hypotheses_kernel, dim3((L.h_cap + INI_WAVES - 1) / INI_WAVES, 2, P), dim3(INI_THREADS), (size_t)L.cap * 16, s, L);
  hipLaunchKernelGGL(initz_select_kernel, dim3(P), dim3(64), 0, s, L);
  hipLaunchKernelGGL(initz_checkrt_kernel, dim3(8, P), dim3(INI_RT_THREADS), 0, s, L);
  hipLaunchKernelGGL(initz_decide_kernel, dim3(P), dim3(INI_RT_THREADS), 0, s, L);
}
