// pnp_kernels.hip -- PnPsolver's RANSAC (L/src/PnPsolver.cc:163-289): every hypothesis of every problem in one launch, the refines
// of the strict prefix maxima in a second, and the sequential rule of iterate (:205-243) applied to counts and refine verdicts in a
// third.  The arithmetic is pnp_internal.h; this file stages, distributes and scans.
//   pnp_hypotheses_kernel  grid (ceil(h_cap / PNP_WAVES), P): a workgroup is PNP_WAVES waves on ONE problem.  It stages the problem's
//     correspondences in LDS once (24 bytes each), then each wave takes one hypothesis: EPnP on its four correspondences with the
//     wave's PnpWork in LDS (MtM and the rotation accumulator, two 12 x 12 doubles, are the bulk of it; nothing is indexed in
//     registers), the Jacobi's six disjoint rotations of a round spread over the lanes, the three starts on three lanes.  Then
//     CheckInliers, a lane per correspondence: the ballot of 64 verdicts IS the inlier word, its popcount goes to the count.
//   pnp_refine_kernel      grid (h_cap, P), one wave: a hypothesis whose count is >= min_inliers and larger than every earlier count is
//     a best-so-far of iterate; the others leave at once.  The set bits of its word row become the index list in LDS, in order, and the
//     same solve and CheckInliers follow on them.
//   pnp_select_kernel      one wave per problem: the first refine that succeeded, else the highest prefix maximum; writes the result
//     record and copies the word row that goes with it.
// No atomics, no scratch; a hypothesis' bytes depend on its problem and its minimal set only.
#include "pnp_internal.h"

#define PNP_THREADS (PNP_WAVES * 64)
static_assert(sizeof(orbfe_pnp_point) == 24 && sizeof(orbfe_pnp_camera) == 16 && sizeof(orbfe_pnp_hypothesis) == 112 &&
              sizeof(orbfe_pnp_refine) == 112 && sizeof(orbfe_pnp_result) == 80 && sizeof(orbfe_pnp_diag) == 640, "record layout");
static_assert(sizeof(PnpWork) == 7016 && PNP_WAVES * sizeof(PnpWork) + ORBFE_PNP_MAX_POINTS * (sizeof(orbfe_pnp_point) + 4) <= 65536,
              "a workgroup's LDS");

__device__ __forceinline__ int pnp_clamp(int v, int cap) { return min(max(v, 0), cap); }

__device__ __forceinline__ PnpCamera pnp_camera(const orbfe_pnp_camera& c) {
  PnpCamera K;
  K.fu = c.fx; K.fv = c.fy; K.uc = c.cx; K.vc = c.cy;
  return K;
}

// the problem's n correspondences into LDS, as dwords (a record is six)
__device__ __forceinline__ void pnp_stage(const orbfe_pnp_point* src, int n, orbfe_pnp_point* dst, int tid, int threads) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (int i = tid; i < n * 6; i += threads) d[i] = s[i];
}

// CheckInliers over all n correspondences by one wave (:291-320); returns the count, lane 0 stores the words
__device__ __forceinline__ int pnp_check_inliers(const PnpWork* w, int winner, const PnpCamera& K, const orbfe_pnp_point* pts, int n,
                                                 uint64_t* words, int lane) {
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = w->st[winner].R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) t[k] = w->st[winner].t[k];
  int count = 0;
  const int n_words = (n + 63) >> 6;
  for (int wd = 0; wd < n_words; wd++) {
    const int i = wd * 64 + lane;
    bool ok = false;
    if (i < n) ok = pnp_is_inlier(R, t, K, pts[i], nullptr);
    const uint64_t b = __ballot(ok);   // lanes behind n vote 0: the tail bits of the last word are zero
    if (lane == 0) words[wd] = b;
    count += __popcll(b);
  }
  return count;
}

__device__ __forceinline__ void pnp_store_pose(const PnpWork* w, int winner, double* R, double* t) {
  for (int k = 0; k < 9; k++) R[k] = w->st[winner].R[k];
  for (int k = 0; k < 3; k++) t[k] = w->st[winner].t[k];
}

__global__ __launch_bounds__(PNP_THREADS) void pnp_hypotheses_kernel(PnpLaunch L) {
  extern __shared__ double pnp_lds[];   // PnpWork[PNP_WAVES], orbfe_pnp_point[cap], int32 sel[PNP_WAVES][4]
  const int p = blockIdx.y, cap = L.cap;
  const int n = pnp_clamp(L.n[p], cap), H = pnp_clamp(L.H[p], L.h_cap);
  if (n < 4 || n < L.min_inliers[p] || (int)blockIdx.x * PNP_WAVES >= H) return;   // uniform: nothing is evaluated (:171-174)
  PnpWork* works = reinterpret_cast<PnpWork*>(pnp_lds);
  orbfe_pnp_point* pts = reinterpret_cast<orbfe_pnp_point*>(works + PNP_WAVES);
  int32_t* sels = reinterpret_cast<int32_t*>(pts + cap);
  pnp_stage(L.points + (size_t)p * cap, n, pts, threadIdx.x, PNP_THREADS);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int h = (int)blockIdx.x * PNP_WAVES + wave;
  if (h >= H) return;
  const size_t row = (size_t)p * L.h_cap + h;
  const int W = (cap + 63) >> 6, n_words = (n + 63) >> 6;
  uint64_t* words = L.words + row * W;
  orbfe_pnp_hypothesis* rec = L.hyps + row;
  const int i0 = L.sets[row * 4], i1 = L.sets[row * 4 + 1], i2 = L.sets[row * 4 + 2], i3 = L.sets[row * 4 + 3];
  if (!pnp_set_ok(i0, i1, i2, i3, n)) {   // not a draw of :187-197: an all-zero record, nothing outside the problem is read
    for (int wd = lane; wd < n_words; wd += 64) words[wd] = 0;
    uint32_t* r32 = reinterpret_cast<uint32_t*>(rec);
    if (lane < 28) r32[lane] = lane == 26 ? 0xffffffffu : 0u;   // refine = -1
    return;
  }
  PnpWork* w = works + wave;
  int32_t* sel = sels + 4 * wave;
  if (lane == 0) { sel[0] = i0; sel[1] = i1; sel[2] = i2; sel[3] = i3; }
  PNP_SYNC();
  const PnpCamera K = pnp_camera(L.camera[p]);
  const int winner = pnp_compute_pose(w, K, pts, sel, 4, lane, 64);
  const int count = pnp_check_inliers(w, winner, K, pts, n, words, lane);
  if (lane == 0) {
    pnp_store_pose(w, winner, rec->R, rec->t);
    rec->n_inliers = count; rec->winner = winner; rec->refine = -1; rec->reserved = 0;
    if (L.diag) pnp_fill_diag(w, L.diag + row);
  }
}

__global__ __launch_bounds__(64) void pnp_refine_kernel(PnpLaunch L) {
  extern __shared__ double pnp_lds[];   // PnpWork, orbfe_pnp_point[cap], int32 sel[cap]
  const int p = blockIdx.y, h = blockIdx.x, cap = L.cap, lane = threadIdx.x;
  const int n = pnp_clamp(L.n[p], cap), H = pnp_clamp(L.H[p], L.h_cap), min_inliers = L.min_inliers[p];
  if (n < 4 || n < min_inliers || h >= H) return;
  const size_t row = (size_t)p * L.h_cap + h;
  const orbfe_pnp_hypothesis* hyps = L.hyps + (size_t)p * L.h_cap;
  const int c = hyps[h].n_inliers;
  if (c < min_inliers || c < 4) return;   // :205 (a refine on fewer than four correspondences cannot come from the reference's parameters)
  int prev = 0;                           // mnBestInliers before this iteration
  for (int j = lane; j < h; j += 64) prev = max(prev, hyps[j].n_inliers);
  for (int d = 32; d > 0; d >>= 1) prev = max(prev, __shfl_xor(prev, d));
  if (!(c > prev)) return;                // :207: not a new best, its Refine() repeats an earlier one
  PnpWork* w = reinterpret_cast<PnpWork*>(pnp_lds);
  orbfe_pnp_point* pts = reinterpret_cast<orbfe_pnp_point*>(w + 1);
  int32_t* sel = reinterpret_cast<int32_t*>(pts + cap);
  pnp_stage(L.points + (size_t)p * cap, n, pts, lane, 64);
  const int W = (cap + 63) >> 6, n_words = (n + 63) >> 6;
  const uint64_t* src = L.words + row * W;
  int m = 0;
  for (int wd = 0; wd < n_words; wd++) {   // vIndices (:252-256): the set bits in order
    const uint64_t b = src[wd];
    if ((b >> lane) & 1) {
      const int at = m + __popcll(b & ((1ull << lane) - 1ull));
      if (at < cap) sel[at] = wd * 64 + lane;   // a word row is the hypothesis kernel's: bits behind n are zero
    }
    m += __popcll(b);
  }
  m = min(m, n);
  PNP_SYNC();
  if (m < 4) return;
  const PnpCamera K = pnp_camera(L.camera[p]);
  const int winner = pnp_compute_pose(w, K, pts, sel, m, lane, 64);
  const int count = pnp_check_inliers(w, winner, K, pts, n, L.refine_words + row * W, lane);
  if (lane == 0) {
    orbfe_pnp_refine* rec = L.refines + row;
    pnp_store_pose(w, winner, rec->R, rec->t);
    rec->n_inliers = count; rec->success = count > min_inliers ? 1 : 0; rec->winner = winner; rec->n_used = m;
    L.hyps[row].refine = h;
    if (L.refine_diag) pnp_fill_diag(w, L.refine_diag + row);
  }
}

__global__ __launch_bounds__(64) void pnp_select_kernel(PnpLaunch L) {
  const int p = blockIdx.x, lane = threadIdx.x, cap = L.cap;
  const int n = pnp_clamp(L.n[p], cap), H = pnp_clamp(L.H[p], L.h_cap), min_inliers = L.min_inliers[p];
  const int W = (cap + 63) >> 6, n_words = (n + 63) >> 6;
  const orbfe_pnp_hypothesis* hyps = L.hyps + (size_t)p * L.h_cap;
  const orbfe_pnp_refine* refines = L.refines + (size_t)p * L.h_cap;
  int returned = -1, best = -1;
  if (!(n < 4 || n < min_inliers)) {
    for (int base = 0; base < H; base += 64) {
      const int h = base + lane;
      const bool is_best = h < H && hyps[h].refine == h;
      const bool ok = is_best && refines[h].success != 0;
      const uint64_t won = __ballot(ok), bests = __ballot(is_best);
      if (won) {   // :220-228: the first successful refine ends the search; the best is the prefix maximum it ran on
        returned = base + __ffsll((unsigned long long)won) - 1;
        best = returned;
        break;
      }
      if (bests) best = base + 63 - __clzll((unsigned long long)bests);
    }
  }
  const bool refined = returned >= 0;
  if (!refined) returned = best;   // :232-242: at exhaustion the best hypothesis, whose count is >= min_inliers by construction
  if (lane == 0) {
    orbfe_pnp_result r;
    uint32_t* rw = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (int k = 0; k < 20; k++) rw[k] = 0u;
    r.returned = returned; r.refined = refined ? 1 : 0; r.best = best;
    if (best >= 0) {
      r.best_inliers = hyps[best].n_inliers;
      const double* R = refined ? refines[best].R : hyps[best].R;
      const double* t = refined ? refines[best].t : hyps[best].t;
      r.n_inliers = refined ? refines[best].n_inliers : hyps[best].n_inliers;
#pragma unroll
      for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) r.Tcw[4 * i + j] = (float)R[3 * i + j];   // convertTo(CV_32F) (:213-217, :280-284)
        r.Tcw[4 * i + 3] = (float)t[i];
      }
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(L.result + p);
#pragma unroll
    for (int k = 0; k < 20; k++) out[k] = rw[k];
  }
  const uint64_t* src = (refined ? L.refine_words : L.words) + ((size_t)p * L.h_cap + (best >= 0 ? best : 0)) * W;
  for (int wd = lane; wd < n_words; wd += 64) L.mask[(size_t)p * W + wd] = best >= 0 ? src[wd] : 0;
}

void orbfe_launch_pnp_hypotheses(const PnpLaunch& L, int P, hipStream_t s) {
  if (P < 1 || L.h_cap < 1 || L.cap < 1) return;
  hipLaunchKernelGGL(pnp_hypotheses_kernel, dim3((L.h_cap + PNP_WAVES - 1) / PNP_WAVES, P), dim3(PNP_THREADS),
                     PNP_WAVES * sizeof(PnpWork) + (size_t)L.cap * sizeof(orbfe_pnp_point) + PNP_WAVES * 16, s, L);
}

void orbfe_launch_pnp_refine(const PnpLaunch& L, int P, hipStream_t s) {
  if (P < 1 || L.h_cap < 1 || L.cap < 1) return;
  hipLaunchKernelGGL(pnp_refine_kernel, dim3(L.h_cap, P), dim3(64), sizeof(PnpWork) + (size_t)L.cap * (sizeof(orbfe_pnp_point) + 4), s, L);
}

void orbfe_launch_pnp_select(const PnpLaunch& L, int P, hipStream_t s) {
  if (P < 1) return;
  hipLaunchKernelGGL(pnp_select_kernel, dim3(P), dim3(64), 0, s, L);
}
