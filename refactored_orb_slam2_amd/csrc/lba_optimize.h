// lba_optimize.h -- the choreography of ONE g2o optimize() call over a problem of BlockSolver_6_3, for the kernels that run it:
// lba_kernel (lba_kernels.hip: two calls with a classification between them) and ba_kernel (ba_kernels.hip: one call of n
// iterations).  Device code only, every function inlined into the kernel that calls it.  The arithmetic is lba_internal.h's, one
// item per call, and the Levenberg rules are lm_internal.h's; what is stated here is who does which item and where the barriers are.
//
// One workgroup of 256 threads per problem (four waves, one per SIMD: the point pass holds about 70 doubles per lane, and
// profiles/pose_optimization.md records what 1 024 threads do to such a kernel).  The workgroup builds its own plan from the edge
// list -- which must come point by point, keyframes ascending -- in its workspace: the edge range of every point, and for every
// free keyframe the list of its edges, which then ascends in its points.  Work is spread as follows, and every sum has ONE owner who
// walks a list in its order, so no atomics exist and a problem's bytes depend on nothing but its own rows:
//   build      a lane per point: errors, Huber, both Jacobians, Hll and bl in registers, per edge Hpl and its keyframe's share to HBM;
//              then a lane per (free keyframe, entry of Hpp | bp) over that keyframe's edges
//   trial      a lane per point: (Hll + lambda I)^-1, Dinv bl, Hpl Dinv per edge; a lane per row of bschur; a lane per entry of
//              Hschur, walking the two keyframes' edge lists side by side; the dense L L^T across the workgroup, a column at a time
//              (scale the column | barrier | update the trailing matrix | barrier) on the reduced matrix in HBM; the two
//              triangular solves with the vectors in LDS, one barrier per column; a lane per point for the back-substitution and the
//              update, a lane per keyframe for exp(x) * pose; a lane per point for the trial's chi2
//   control    chi2, computeScale (lm_reduce.h) and every count land in LDS; each lane repeats the few operations of the Levenberg
//              bookkeeping on those identical values, so control flow is uniform over the workgroup by construction
// LDS holds what every pass re-reads: the poses, the saved poses, the row-block maps, the vectors of the solve and the reduction
// buffers (43 KB).  The reduced matrix, the per-point and the per-edge blocks are the problem's workspace in HBM.
#pragma once
#include "lba_internal.h"
#include "lm_reduce.h"

#define LBA_THREADS 256
#define LBA_WAVES (LBA_THREADS / 64)
#define LBA_NMAX (6 * ORBFE_LBA_MAX_FREE)

struct LbaShared {   // one per workgroup, in LDS
  PoseSE3 pose[ORBFE_LBA_MAX_KEYFRAMES], bak[ORBFE_LBA_MAX_KEYFRAMES];
  int slot[ORBFE_LBA_MAX_KEYFRAMES];
  int kf_of_fi[ORBFE_LBA_MAX_FREE], kf_start[ORBFE_LBA_MAX_FREE + 1], fi_of_slot[ORBFE_LBA_MAX_FREE], cnt[ORBFE_LBA_MAX_FREE];
  double b[LBA_NMAX], y[LBA_NMAX], x[LBA_NMAX], diag[LBA_NMAX];
  double red[LBA_WAVES * 2], tot[2], red_m[LBA_WAVES];
  int red_i[LBA_WAVES];
  int ns, nfree;
};

struct LbaCall {   // what one optimize() call reports
  int iterations, trials;
  double chi2_first, chi2_final;
};

enum { LBA_UNADDRESSABLE = -2, LBA_REFUSED = -1, LBA_IDLE = 0, LBA_READY = 1 };

// Problem blockIdx.x of the launch: its arrays into W, the estimates widened into LDS, the plan into the workspace.  Uniform over the
// workgroup.  LBA_UNADDRESSABLE: the counts are negative or exceed the caps, nothing was read or written.  LBA_REFUSED (too many
// free keyframes, an edge list that breaks a rule) and LBA_IDLE (no free keyframe, or no edge): poses and points have gone through
// as they are; W.n_free and W.n_e are set.  LBA_READY: every edge is at level 0
__device__ __forceinline__ int lba_prepare(const LbaLaunch& L, const orbfe_lba_problem& Q, LbaShared& sh, LbaWs& W) {
  const int tid = threadIdx.x;
  if (Q.n_kf < 0 || Q.n_kf > L.kf_cap || Q.n_points < 0 || Q.n_points > L.point_cap || Q.n_edges < 0 || Q.n_edges > L.edge_cap ||
      Q.kf_offset < 0 || Q.point_offset < 0 || Q.edge_offset < 0)   // nothing of such a problem can be addressed
    return LBA_UNADDRESSABLE;
  const int F = L.kf_cap < ORBFE_LBA_MAX_FREE ? L.kf_cap : ORBFE_LBA_MAX_FREE;
  lba_ws_carve(L.workspace + (size_t)blockIdx.x * lba_ws_bytes(F, L.point_cap, L.edge_cap), F, L.point_cap, L.edge_cap, W);
  W.n_kf = Q.n_kf;
  W.n_pt = Q.n_points;
  W.n_e = Q.n_edges;
  W.edges = L.edges + Q.edge_offset;
  W.K.fx = (double)L.camera->fx;
  W.K.fy = (double)L.camera->fy;
  W.K.cx = (double)L.camera->cx;
  W.K.cy = (double)L.camera->cy;
  W.K.bf = (double)L.camera->mbf;
  W.pose = sh.pose;
  W.pose_bak = sh.bak;
  W.slot_of_kf = sh.slot;
  W.kf_of_fi = sh.kf_of_fi;
  W.kf_start = sh.kf_start;
  W.fi_of_slot = sh.fi_of_slot;
  const float* poses_in = L.poses + (size_t)Q.kf_offset * 12;
  const uint8_t* fixed = L.fixed + Q.kf_offset;
  const uint8_t* points_in = L.points + (size_t)Q.point_offset * L.point_stride;

  // the free keyframes, and whether the edge list can be walked at all
  if (tid == 0) {
    int nf = 0;
    for (int k = 0; k < W.n_kf; k++)
      if (!fixed[k]) {
        if (nf < ORBFE_LBA_MAX_FREE) sh.kf_of_fi[nf] = k;
        nf++;
      }
    sh.nfree = nf;
  }
  int invalid = 0;
  for (int i = tid; i < W.n_e; i += LBA_THREADS) invalid += lba_edge_valid(W.edges, i, W.n_kf, W.n_pt) ? 0 : 1;
  invalid = lm_reduce_count<LBA_WAVES>(invalid, sh.red_i, tid);
  W.n_free = sh.nfree;
  const bool refused = invalid > 0 || W.n_free > ORBFE_LBA_MAX_FREE;
  if (refused || W.n_free == 0 || W.n_e == 0) {   // uniform: the inputs go through as they are
    float* poses_out = L.poses_out + (size_t)Q.kf_offset * 12;
    float* points_out = L.points_out + (size_t)Q.point_offset * 3;
    for (int j = tid; j < W.n_kf * 12; j += LBA_THREADS) poses_out[j] = poses_in[j];
    for (int j = tid; j < W.n_pt * 3; j += LBA_THREADS)
      points_out[j] = reinterpret_cast<const float*>(points_in + (size_t)(j / 3) * L.point_stride)[j % 3];
    return refused ? LBA_REFUSED : LBA_IDLE;
  }

  // the estimates, widened once; the plan
  for (int k = tid; k < W.n_kf; k += LBA_THREADS) {
    sh.pose[k] = pose_from_Tcw(poses_in + (size_t)k * 12);
    sh.slot[k] = -1;
  }
  for (int p = tid; p < W.n_pt; p += LBA_THREADS) {
    const float* X = reinterpret_cast<const float*>(points_in + (size_t)p * L.point_stride);
    W.pt[3 * p] = (double)X[0];
    W.pt[3 * p + 1] = (double)X[1];
    W.pt[3 * p + 2] = (double)X[2];
    W.pt_start[p] = 0;
    W.pt_end[p] = 0;
    W.pt_active[p] = 0;
  }
  __syncthreads();
  for (int i = tid; i < W.n_e; i += LBA_THREADS) {
    const int p = W.edges[i].point;
    if (i == 0 || W.edges[i - 1].point != p) W.pt_start[p] = i;
    if (i == W.n_e - 1 || W.edges[i + 1].point != p) W.pt_end[p] = i + 1;
    W.level[i] = 0;
    W.chi2[i] = 0.0;
  }
  if (tid < W.n_free) {   // every lane reads the same edge: one broadcast load per step
    const int kf = sh.kf_of_fi[tid];
    int c = 0;
    for (int i = 0; i < W.n_e; i++) c += W.edges[i].kf == kf ? 1 : 0;
    sh.cnt[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int fi = 0; fi < W.n_free; fi++) {
      sh.kf_start[fi] = o;
      o += sh.cnt[fi];
    }
    sh.kf_start[W.n_free] = o;
  }
  __syncthreads();
  if (tid < W.n_free) {
    const int kf = sh.kf_of_fi[tid];
    int o = sh.kf_start[tid];
    for (int i = 0; i < W.n_e; i++)
      if (W.edges[i].kf == kf) W.kf_list[o++] = i;
  }
  __syncthreads();
  return LBA_READY;
}

// initializeOptimization(0) and optimize(max_it) over the level-0 edges, the Huber kernel on every edge iff `robust`, with delta_mono
// on a monocular edge.  Uniform over the workgroup; ends behind a barrier
__device__ __forceinline__ void lba_optimize_call(const LbaWs& W, LbaShared& sh, bool robust, double delta_mono, int max_it, LbaCall& call) {
  const int tid = threadIdx.x;
  // initializeOptimization(0): a free keyframe with a level-0 edge has a row block
  if (tid < W.n_free) {
    int c = 0;
    for (int q = sh.kf_start[tid]; q < sh.kf_start[tid + 1]; q++) c += W.level[W.kf_list[q]] ? 0 : 1;
    sh.cnt[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int ns = 0;
    for (int fi = 0; fi < W.n_free; fi++) {
      const int kf = sh.kf_of_fi[fi];
      if (sh.cnt[fi] > 0) {
        sh.fi_of_slot[ns] = fi;
        sh.slot[kf] = ns++;
      } else {
        sh.slot[kf] = -1;
      }
    }
    sh.ns = ns;
  }
  __syncthreads();
  const int ns = sh.ns, n = 6 * ns;
  LmState lm;
  lm.lambda = 0.0;
  lm.ni = 2.0;
  double current_chi = 0.0;
  int iterations = 0, trials = 0;
  call.chi2_first = 0.0;
  for (int it = 0; it < max_it; it++) {
    double v[2] = {0.0, 0.0};
    double maxd = 0.0;
    for (int p = tid; p < W.n_pt; p += LBA_THREADS) lba_point_build(W, p, robust, &v[0], &maxd, delta_mono);
    __syncthreads();
    for (int t = tid; t < ns * LBA_EKF; t += LBA_THREADS) {
      const int k = t % LBA_EKF;
      const double s = lba_kf_sum(W, sh.fi_of_slot[t / LBA_EKF], k);
      if (lba_is_diag(k)) maxd = fmax(fabs(s), maxd);
    }
    lm_reduce<1, 2, LBA_WAVES>(v, sh.red, sh.tot, tid);
    current_chi = sh.tot[0];
    if (it == 0) {   // computeLambdaInit over every active vertex
      maxd = lm_reduce_max<LBA_WAVES>(maxd, sh.red_m, tid);
      lm.lambda = 1e-5 * maxd;
      lm.ni = 2.0;
      call.chi2_first = current_chi;
    }
    double rho = 0.0;
    int qmax = 0;
    do {
      const double lambda = lm.lambda;
      for (int p = tid; p < W.n_pt; p += LBA_THREADS) lba_point_dinv(W, p, lambda);
      __syncthreads();
      for (int t = tid; t < n; t += LBA_THREADS) sh.b[t] = lba_bschur(W, sh.fi_of_slot[t / 6], t % 6);
      for (int t = tid; t < ns * ns * 36; t += LBA_THREADS) {
        const int i = t / (ns * 36), rem = t % (ns * 36);
        const int j = rem / 36, r = (rem % 36) / 6, c = rem % 6;
        if (j < i || (i == j && r > c)) continue;
        W.S[(size_t)(6 * j + c) * n + (6 * i + r)] = lba_schur_entry(W, sh.fi_of_slot[i], sh.fi_of_slot[j], r, c, lambda);
      }
      __syncthreads();
      // L L^T, a column at a time; S keeps its diagonal, L's goes to LDS
      bool ok2 = true;
      for (int k = 0; k < n; k++) {
        const double d = W.S[(size_t)k * n + k];
        if (!(d > 0.0)) {   // uniform: every lane read the same value
          ok2 = false;
          break;
        }
        const double lkk = sqrt(d);
        if (tid == 0) sh.diag[k] = lkk;
        for (int i = k + 1 + tid; i < n; i += LBA_THREADS) W.S[(size_t)i * n + k] = W.S[(size_t)i * n + k] / lkk;
        __syncthreads();
        for (int i = k + 1 + (tid >> 4); i < n; i += LBA_THREADS / 16) {
          const double lik = W.S[(size_t)i * n + k];
          for (int j = k + 1 + (tid & 15); j <= i; j += 16) W.S[(size_t)i * n + j] -= lik * W.S[(size_t)j * n + k];
        }
        __syncthreads();
      }
      double temp_chi = 0.0, scale = 0.0;
      if (ok2) {   // uniform
        // L y = b, then L^T x = y: element i belongs to lane i mod 256, the solved entry is handed over through LDS
        for (int k = 0; k < n; k++) {
          if (tid == (k & (LBA_THREADS - 1))) sh.y[k] = sh.b[k] / sh.diag[k];
          __syncthreads();
          const double yk = sh.y[k];
          for (int i = tid; i < n; i += LBA_THREADS)
            if (i > k) sh.b[i] -= W.S[(size_t)i * n + k] * yk;
        }
        for (int k = n - 1; k >= 0; k--) {
          if (tid == (k & (LBA_THREADS - 1))) sh.x[k] = sh.y[k] / sh.diag[k];
          __syncthreads();
          const double xk = sh.x[k];
          for (int i = tid; i < n; i += LBA_THREADS)
            if (i < k) sh.y[i] -= W.S[(size_t)k * n + i] * xk;
        }
        __syncthreads();
        double u[2] = {0.0, 0.0};   // the trial's chi2, computeScale
        for (int p = tid; p < W.n_pt; p += LBA_THREADS) lba_point_update(W, p, lambda, sh.x, &u[1]);
        if (tid < ns) lba_pose_update(W, tid, lambda, sh.x, &u[1]);
        __syncthreads();
        for (int p = tid; p < W.n_pt; p += LBA_THREADS) lba_point_chi(W, p, robust, &u[0], delta_mono);
        lm_reduce<2, 2, LBA_WAVES>(u, sh.red, sh.tot, tid);
        temp_chi = sh.tot[0];
        scale = sh.tot[1];
      }
      trials++;
      if (lm_trial_scaled(lm, ok2, current_chi, temp_chi, scale, &rho)) {
        current_chi = temp_chi;
      } else {
        if (ok2) {   // pop
          for (int p = tid; p < W.n_pt; p += LBA_THREADS) lba_point_pop(W, p);
          if (tid < ns) {
            const int kf = sh.kf_of_fi[sh.fi_of_slot[tid]];
            sh.pose[kf] = sh.bak[kf];
          }
        }
        if (!isfinite(lm.lambda)) break;
      }
      __syncthreads();
      qmax++;
    } while (rho < 0 && qmax < 10);
    __syncthreads();
    iterations++;
    if (qmax == 10 || rho == 0 || !isfinite(lm.lambda)) break;   // Terminate
  }
  call.iterations = iterations;
  call.trials = trials;
  call.chi2_final = current_chi;
}

// The estimates of a problem that ran: a free keyframe's pose as Converter::toCvMat(SE3Quat) rounds it; a fixed one's bytes as given
// (LocalBundleAdjustment writes back the local keyframes only) unless fixed_too (BundleAdjustment writes back every vertex); a point
// without an edge as given
__device__ __forceinline__ void lba_write_estimates(const LbaLaunch& L, const orbfe_lba_problem& Q, const LbaShared& sh, const LbaWs& W,
                                                    bool fixed_too) {
  const int tid = threadIdx.x;
  const float* poses_in = L.poses + (size_t)Q.kf_offset * 12;
  const uint8_t* fixed = L.fixed + Q.kf_offset;
  const uint8_t* points_in = L.points + (size_t)Q.point_offset * L.point_stride;
  float* poses_out = L.poses_out + (size_t)Q.kf_offset * 12;
  float* points_out = L.points_out + (size_t)Q.point_offset * 3;
  for (int k = tid; k < W.n_kf; k += LBA_THREADS) {
    if (fixed[k] && !fixed_too) {
#pragma unroll
      for (int j = 0; j < 12; j++) poses_out[(size_t)k * 12 + j] = poses_in[(size_t)k * 12 + j];
    } else {
      float T[12];
      pose_to_Tcw(sh.pose[k], T);
#pragma unroll
      for (int j = 0; j < 12; j++) poses_out[(size_t)k * 12 + j] = T[j];
    }
  }
  for (int p = tid; p < W.n_pt; p += LBA_THREADS) {
    const float* X = reinterpret_cast<const float*>(points_in + (size_t)p * L.point_stride);
    const bool seen = W.pt_start[p] < W.pt_end[p];
#pragma unroll
    for (int j = 0; j < 3; j++) points_out[(size_t)p * 3 + j] = seen ? (float)W.pt[3 * p + j] : X[j];
  }
}
