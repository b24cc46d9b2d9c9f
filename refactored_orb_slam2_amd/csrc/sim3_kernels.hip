// sim3_kernels.hip -- Sim3Solver's RANSAC (L/src/Sim3Solver.cc:138-200), every hypothesis of every problem in one launch, and
// the sequential acceptance rule of iterate (:178-193) applied to the counts afterwards.  The arithmetic is sim3_internal.h; this
// file stages, distributes and scans.
//   sim3_hypotheses_kernel  grid (ceil(h_cap / SIM3_WAVES), P): a workgroup is SIM3_WAVES waves on ONE problem.  It first runs the
//     constructor's preparation (:92-96, :106-107) for the problem's correspondences into LDS, 12 planes of `cap` floats (48 bytes a
//     correspondence, at most 48 KiB: ORBFE_SIM3_MAX_PAIRS), so that every later read is a conflict-free ds_read of consecutive
//     lanes or a broadcast.  Preparing again in each of the problem's workgroups costs n / 256 rows a thread and saves a kernel, a
//     workspace argument of the device form and a round trip through L2.  Then each wave takes one hypothesis: the Horn solution
//     is wave-uniform (all lanes read the same three rows), is computed once per wave -- 64 lanes in lockstep cost what one costs --
//     and moved into SGPRs by readfirstlane, so the per-correspondence loop holds only its own row in VGPRs.  Lanes stride over the
//     correspondences; the ballot of 64 verdicts IS the inlier word, stored by lane 0, its popcount goes to the count.
//   sim3_select_kernel      one wave per problem: first count > min_inliers, else the last maximum; writes the result record and
//     copies that hypothesis' words to the result mask.
// No atomics, no scratch; a hypothesis' bytes depend on its problem and its triple only, so they do not depend on H, P or the
// position in the batch.
#include "sim3_internal.h"

#define SIM3_THREADS (SIM3_WAVES * 64)
static_assert(sizeof(orbfe_sim3_view) == 64 && sizeof(orbfe_sim3_pair) == 32 && sizeof(orbfe_sim3_hypothesis) == 64 &&
              sizeof(orbfe_sim3_result) == 128 && sizeof(Sim3Prepared) == 48, "record layout");

__device__ __forceinline__ int sim3_clamp(int v, int cap) { return min(max(v, 0), cap); }
__device__ __forceinline__ float sim3_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

__global__ __launch_bounds__(SIM3_THREADS) void sim3_hypotheses_kernel(Sim3Launch L) {
  extern __shared__ float prep[];   // [12][cap]
  const int p = blockIdx.y, cap = L.cap;
  const int n = sim3_clamp(L.n[p], cap), H = sim3_clamp(L.H[p], L.h_cap);
  if (n < 3 || n < L.min_inliers[p] || (int)blockIdx.x * SIM3_WAVES >= H) return;   // uniform: nothing is evaluated (:144-147)
  const orbfe_sim3_view& V1 = L.view1[p];
  const orbfe_sim3_view& V2 = L.view2[p];
  for (int i = threadIdx.x; i < n; i += SIM3_THREADS) {
    const orbfe_sim3_pair pr = L.pairs[(size_t)p * cap + i];
    Sim3Prepared q;
    sim3_prepare(V1, V2, pr, q);
    prep[i] = q.c1[0]; prep[cap + i] = q.c1[1]; prep[2 * cap + i] = q.c1[2];
    prep[3 * cap + i] = q.c2[0]; prep[4 * cap + i] = q.c2[1]; prep[5 * cap + i] = q.c2[2];
    prep[6 * cap + i] = q.im1[0]; prep[7 * cap + i] = q.im1[1]; prep[8 * cap + i] = q.im2[0]; prep[9 * cap + i] = q.im2[1];
    prep[10 * cap + i] = q.max_err1; prep[11 * cap + i] = q.max_err2;
  }
  __syncthreads();
  const int h = (int)blockIdx.x * SIM3_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (h >= H) return;
  const size_t row = (size_t)p * L.h_cap + h;
  const int W = (cap + 63) >> 6, n_words = (n + 63) >> 6;
  uint64_t* words = L.words + row * W;
  uint32_t* rec = reinterpret_cast<uint32_t*>(L.hyps + row);
  const int i0 = L.triples[row * 3], i1 = L.triples[row * 3 + 1], i2 = L.triples[row * 3 + 2];
  if (!sim3_triple_ok(i0, i1, i2, n)) {   // not a draw of :162-172: an all-zero record, nothing outside the problem is read
    for (int w = lane; w < n_words; w += 64) words[w] = 0;
    if (lane < 16) rec[lane] = 0u;
    return;
  }
  float sR[9], t[3], sRinv[9], tinv[3], R[9], s;
  {
    const float a1[3] = {prep[i0], prep[cap + i0], prep[2 * cap + i0]}, a2[3] = {prep[3 * cap + i0], prep[4 * cap + i0], prep[5 * cap + i0]};
    const float b1[3] = {prep[i1], prep[cap + i1], prep[2 * cap + i1]}, b2[3] = {prep[3 * cap + i1], prep[4 * cap + i1], prep[5 * cap + i1]};
    const float c1[3] = {prep[i2], prep[cap + i2], prep[2 * cap + i2]}, c2[3] = {prep[3 * cap + i2], prep[4 * cap + i2], prep[5 * cap + i2]};
    Sim3Transform T;
    sim3_horn(a1, b1, c1, a2, b2, c2, L.fix_scale[p] != 0, T);
    s = sim3_uniform(T.s);
#pragma unroll
    for (int k = 0; k < 9; k++) {
      R[k] = sim3_uniform(T.R[k]); sR[k] = sim3_uniform(T.sR[k]); sRinv[k] = sim3_uniform(T.sRinv[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      t[k] = sim3_uniform(T.t[k]); tinv[k] = sim3_uniform(T.tinv[k]);
    }
  }
  int count = 0;
  for (int w = 0; w < n_words; w++) {
    const int i = w * 64 + lane;
    bool ok = false;
    if (i < n) {
      Sim3Prepared q;
      q.c1[0] = prep[i]; q.c1[1] = prep[cap + i]; q.c1[2] = prep[2 * cap + i];
      q.c2[0] = prep[3 * cap + i]; q.c2[1] = prep[4 * cap + i]; q.c2[2] = prep[5 * cap + i];
      q.im1[0] = prep[6 * cap + i]; q.im1[1] = prep[7 * cap + i]; q.im2[0] = prep[8 * cap + i]; q.im2[1] = prep[9 * cap + i];
      q.max_err1 = prep[10 * cap + i]; q.max_err2 = prep[11 * cap + i];
      ok = sim3_is_inlier(V1, V2, sR, t, sRinv, tinv, q);
    }
    const uint64_t b = __ballot(ok);   // lanes behind n vote 0: the tail bits of the last word are zero
    if (lane == 0) words[w] = b;
    count += __popcll(b);
  }
  if (lane == 0) {
    rec[0] = __float_as_uint(s);
#pragma unroll
    for (int k = 0; k < 9; k++) rec[1 + k] = __float_as_uint(R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) rec[10 + k] = __float_as_uint(t[k]);
    rec[13] = (uint32_t)count;
    rec[14] = 0u; rec[15] = 0u;
  }
}

__global__ __launch_bounds__(64) void sim3_select_kernel(Sim3Launch L) {
  const int p = blockIdx.x, lane = threadIdx.x, cap = L.cap;
  const int n = sim3_clamp(L.n[p], cap), H = sim3_clamp(L.H[p], L.h_cap), min_inliers = L.min_inliers[p];
  const int W = (cap + 63) >> 6, n_words = (n + 63) >> 6;
  const orbfe_sim3_hypothesis* hyps = L.hyps + (size_t)p * L.h_cap;
  int returned = -1;
  long long key = -1;   // (count << 32) | index of this lane's last maximum: `>=` at :178 lets a later equal count win
  if (!(n < 3 || n < min_inliers)) {
    for (int base = 0; base < H; base += 64) {
      const int h = base + lane;
      const int c = h < H ? hyps[h].n_inliers : -1;
      const uint64_t above = __ballot(c > min_inliers);
      if (above) {   // :186: the first one in hypothesis order ends the search
        returned = base + __ffsll((unsigned long long)above) - 1;
        break;
      }
      if (c >= 0) key = max(key, ((long long)c << 32) | (long long)h);
    }
  }
  for (int d = 32; d > 0; d >>= 1) key = max(key, __shfl_xor(key, d));
  const int best = returned >= 0 ? returned : (key < 0 ? -1 : (int)(key & 0xffffffffll));
  if (lane == 0) {
    orbfe_sim3_result r;
    uint32_t* rw = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (int k = 0; k < 32; k++) rw[k] = 0u;
    r.returned = returned;
    r.best = best;
    if (best >= 0) {
      const orbfe_sim3_hypothesis hb = hyps[best];
      r.best_inliers = hb.n_inliers;
      r.n_inliers = returned >= 0 ? hb.n_inliers : 0;
      r.s = hb.s;
#pragma unroll
      for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
          r.R[3 * i + j] = hb.R[3 * i + j];
          r.T12[4 * i + j] = hb.s * hb.R[3 * i + j];   // :308, the product the hypothesis was scored with
        }
        r.t[i] = hb.t[i];
        r.T12[4 * i + 3] = hb.t[i];
      }
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(L.result + p);
#pragma unroll
    for (int k = 0; k < 32; k++) out[k] = rw[k];
  }
  const uint64_t* src = L.words + ((size_t)p * L.h_cap + (best >= 0 ? best : 0)) * W;
  for (int w = lane; w < n_words; w += 64) L.mask[(size_t)p * W + w] = best >= 0 ? src[w] : 0;
}

void orbfe_launch_sim3_hypotheses(const Sim3Launch& L, int P, hipStream_t s) {
  if (P < 1 || L.h_cap < 1 || L.cap < 1) return;
  hipLaunchKernelGGL(sim3_hypotheses_kernel, dim3((L.h_cap + SIM3_WAVES - 1) / SIM3_WAVES, P), dim3(SIM3_THREADS),
                     (size_t)L.cap * sizeof(Sim3Prepared), s, L);
}

void orbfe_launch_sim3_select(const Sim3Launch& L, int P, hipStream_t s) {
  if (P < 1) return;
  hipLaunchKernelGGL(sim3_select_kernel, dim3(P), dim3(64), 0, s, L);
}
