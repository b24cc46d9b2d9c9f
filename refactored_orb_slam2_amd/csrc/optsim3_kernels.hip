// optsim3_kernels.hip -- Optimizer::OptimizeSim3 (L/src/Optimizer.cc:1381-1573) for a batch of loop candidates: one 7-DoF similarity
// vertex, two edges per correspondence (x1 = S12 X2 in image 1, x2 = S21 X1 in image 2) with numeric Jacobians, optimize(5), the
// first classification, optimize(10 or 5) on the survivors and the second classification, all inside one launch.  The arithmetic
// is optsim3_internal.h's and, for the optimiser around the edges, lm_internal.h's.
//
// One workgroup of 256 threads per problem.  Lane t owns correspondences t, t + 256, ... and walks them in that order.  The first
// 2 048 are prepared once into LDS as the floats they are (the two camera-frame points of the float gemm, the observations, the two
// weights: 12 floats and a flag byte); a row behind them is re-read and re-prepared from global memory for every evaluation, so no
// per-problem workspace exists and `cap` is bounded by nothing but the library's frame limit.
// Per Levenberg iteration lanes 0 .. 14 of wave 0 build the estimate's 14 perturbed copies (+-1e-9 along each dimension, through
// oplus) and the inverses of all 15 and put them in LDS; every lane then evaluates, per correspondence, the 2 x 15 projections, the
// two 2 x 7 central-difference Jacobians and adds into the 28 upper entries of H, the 7 of b and chi, in double.  Every trial is
// one pass for chi alone.  The sums are lm_reduce.h's, a lane adding e12 before e21: in an order that depends on nothing but the
// problem's own rows, so a problem's result is byte-identical from run to run, at any position in a batch and for any batch size.
// H, b and chi are left in LDS; wave 0 runs the 7 x 7 solve, oplus and the inverse of a trial and hands them to the others
// through LDS; the Levenberg bookkeeping is repeated by every lane on those identical values, so control flow is uniform over the
// workgroup, which is what lets the barriers sit inside the trial loop.  The Jacobian of an edge passes through the lane's own LDS
// slots (an array indexed at run time lives in scratch memory, DESIGN lesson 58).
//
// Deliberate deviation, the pose kernel's: after an optimize() call every correspondence is classified by its
// chi2 at the call's final estimate.  The reference reads the error that the last Levenberg trial left in the edge, also when that
// trial was rejected; such a step is taken at a large lambda and is tiny.
#include "optsim3_internal.h"
#include "lm_reduce.h"

#ifndef OS_THREADS
#define OS_THREADS 256   // 64 and 128 threads were measured against it: profiles/optimize_sim3.md
#endif
#define OS_WAVES (OS_THREADS / 64)
#define OS_LDS_ROWS 2048

struct OsCache {   // flags: 1 = the correspondence was dropped (vpMatches1 entry nulled)
  float x1[OS_LDS_ROWS], y1[OS_LDS_ROWS], z1[OS_LDS_ROWS], x2[OS_LDS_ROWS], y2[OS_LDS_ROWS], z2[OS_LDS_ROWS];
  float u1[OS_LDS_ROWS], v1[OS_LDS_ROWS], u2[OS_LDS_ROWS], v2[OS_LDS_ROWS], w1[OS_LDS_ROWS], w2[OS_LDS_ROWS];
  uint8_t flags[OS_LDS_ROWS];
};

__device__ inline void os_load_global(const orbfe_sim3_view* views, const orbfe_optsim3_pair& p, OsPair& E) {
  float c1[3], c2[3];
  os_prepare(views[0], views[1], p, c1, c2);
  E.x1 = (double)c1[0]; E.y1 = (double)c1[1]; E.z1 = (double)c1[2];
  E.x2 = (double)c2[0]; E.y2 = (double)c2[1]; E.z2 = (double)c2[2];
  E.u1 = (double)p.obs1[0]; E.v1 = (double)p.obs1[1];
  E.u2 = (double)p.obs2[0]; E.v2 = (double)p.obs2[1];
  E.w1 = (double)p.inv_sigma2_1; E.w2 = (double)p.inv_sigma2_2;
}

// correspondence i and whether it was dropped
__device__ inline bool os_pair(const orbfe_sim3_view* views, const orbfe_optsim3_pair* pairs, const uint8_t* bad, const OsCache& C, int i,
                               OsPair& E) {
  if (i < OS_LDS_ROWS) {
    E.x1 = (double)C.x1[i]; E.y1 = (double)C.y1[i]; E.z1 = (double)C.z1[i];
    E.x2 = (double)C.x2[i]; E.y2 = (double)C.y2[i]; E.z2 = (double)C.z2[i];
    E.u1 = (double)C.u1[i]; E.v1 = (double)C.v1[i];
    E.u2 = (double)C.u2[i]; E.v2 = (double)C.v2[i];
    E.w1 = (double)C.w1[i]; E.w2 = (double)C.w2[i];
    return C.flags[i] != 0;
  }
  os_load_global(views, pairs[i], E);
  return bad[i] != 0;
}

// One edge at the 15 transforms T[0 .. 15) into acc: error and chi2 at T[0], column d of the Jacobian from T[1 + 2 d], T[2 + 2 d].
// The loop over the columns is a real loop -- unrolled, the edge's 15 transforms (120 doubles, invariant in the loop over the
// correspondences) are read ahead of that loop, their projections scheduled together, and they spill -- so the 14 entries of the
// Jacobian go through the lane's own LDS slots J[k * OS_THREADS], not through an indexed array.
__device__ inline void os_edge(const OsSim3* T, const OsCam& K, double X, double Y, double Z, double ou, double ov, double w, double delta,
                               double* J, double* acc) {
  double e0, e1;
  os_error(T[0], K, X, Y, Z, ou, ov, &e0, &e1);
#pragma unroll 1
  for (int d = 0; d < 7; d++) {
    double p0, p1, m0, m1;
    os_error(T[1 + 2 * d], K, X, Y, Z, ou, ov, &p0, &p1);
    os_error(T[2 + 2 * d], K, X, Y, Z, ou, ov, &m0, &m1);
    J[(2 * d) * OS_THREADS] = os_central(p0, m0);
    J[(2 * d + 1) * OS_THREADS] = os_central(p1, m1);
  }
  double J0[7], J1[7];
#pragma unroll
  for (int d = 0; d < 7; d++) {
    J0[d] = J[(2 * d) * OS_THREADS];
    J1[d] = J[(2 * d + 1) * OS_THREADS];
  }
  double rho0, rho1;
  lm_huber(os_chi2(e0, e1, w), delta, &rho0, &rho1);
  lm_accumulate<7>(J0, J1, J0, false, e0, e1, 0.0, w, rho0, rho1, acc);   // two rows: the third J0 is a stand-in
}

__device__ inline double os_edge_chi2(const OsSim3& S, const OsCam& K, double X, double Y, double Z, double ou, double ov, double w) {
  double e0, e1;
  os_error(S, K, X, Y, Z, ou, ov, &e0, &e1);
  return os_chi2(e0, e1, w);
}

__device__ inline void os_set_transform(orbfe_optsim3_result& r, const float* v) {
  r.s = v[0];
#pragma unroll
  for (int j = 0; j < 9; j++) r.R[j] = v[1 + j];
#pragma unroll
  for (int j = 0; j < 3; j++) r.t[j] = v[10 + j];
}

__global__ __launch_bounds__(OS_THREADS) void optimize_sim3_kernel(OsLaunch L) {
  __shared__ double red[OS_WAVES * OS_NACC];
  __shared__ double Hb[OS_NACC];   // H (28), b (7), chi of the iteration
  __shared__ double chi_t;         // chi of the trial
  __shared__ double sh_x[7];       // the trial's update, estimate, its inverse and whether the solve succeeded
  __shared__ OsSim3 sh_trial[2];
  __shared__ int sh_ok;
  __shared__ OsSim3 sh_T[2 * OS_NTRANSFORMS];   // the estimate and its perturbed copies, then their inverses
  __shared__ double sh_J[14 * OS_THREADS];      // a lane's Jacobian: entries tid + k * OS_THREADS
  __shared__ int red_i[OS_WAVES];
  __shared__ orbfe_sim3_view views[2];
  __shared__ OsCache cache;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(L.n[p], 0), L.cap);
  const size_t row0 = (size_t)p * L.cap;
  const orbfe_optsim3_pair* pairs = L.pairs + row0;
  uint8_t* bad = L.bad + row0;
  const float* in = L.s_R_t_in + (size_t)p * 13;
  const bool fix_scale = L.fix_scale[p] != 0;
  const float th2f = L.th2[p];
  const double th2 = (double)th2f, delta = os_delta(th2f);
  orbfe_optsim3_result res;
  os_set_transform(res, in);
  res.n_pairs = n;
  res.n_bad = 0;
  res.n_inliers = 0;
  res.iterations[0] = res.iterations[1] = 0;
  res.reserved[0] = res.reserved[1] = 0;
  if (n == 0) {   // no edge: optimize() does nothing and 0 - 0 < 10
    if (tid == 0) L.result[p] = res;
    return;
  }
  if (tid < 16)   // orbfe_sim3_view: 16 floats
    reinterpret_cast<float*>(views)[tid] = reinterpret_cast<const float*>(L.view1 + p)[tid];
  else if (tid < 32)
    reinterpret_cast<float*>(views)[tid] = reinterpret_cast<const float*>(L.view2 + p)[tid - 16];
  __syncthreads();
  OsCam K1, K2;
  K1.fx = (double)views[0].fx; K1.fy = (double)views[0].fy; K1.cx = (double)views[0].cx; K1.cy = (double)views[0].cy;
  K2.fx = (double)views[1].fx; K2.fy = (double)views[1].fy; K2.cx = (double)views[1].cx; K2.cy = (double)views[1].cy;
  for (int i = tid; i < n; i += OS_THREADS) {
    bad[i] = 0;
    if (i < OS_LDS_ROWS) {   // the float values as they came: every widening is exact
      const orbfe_optsim3_pair q = pairs[i];
      float c1[3], c2[3];
      os_prepare(views[0], views[1], q, c1, c2);
      cache.x1[i] = c1[0]; cache.y1[i] = c1[1]; cache.z1[i] = c1[2];
      cache.x2[i] = c2[0]; cache.y2[i] = c2[1]; cache.z2[i] = c2[2];
      cache.u1[i] = q.obs1[0]; cache.v1[i] = q.obs1[1];
      cache.u2[i] = q.obs2[0]; cache.v2[i] = q.obs2[1];
      cache.w1[i] = q.inv_sigma2_1; cache.w2[i] = q.inv_sigma2_2;
      cache.flags[i] = 0;
    }
  }
  __syncthreads();

  OsSim3 S = os_from_floats(in);
  int n_bad = 0;
  for (int call = 0; call < 2; call++) {
    const int max_its = call == 0 ? 5 : (n_bad > 0 ? 10 : 5);   // Optimizer.cc:1518, :1539-1551
    LmState lm;
    lm.lambda = 0.0;
    lm.ni = 2.0;
    int its = 0;
    for (int it = 0; it < max_its; it++) {
      if (tid < OS_NTRANSFORMS) {   // the readers of the iteration before passed the barriers of its reductions
        const OsSim3 T = os_perturbed(S, tid, fix_scale);
        sh_T[tid] = T;
        sh_T[OS_NTRANSFORMS + tid] = os_inverse(T);
      }
      __syncthreads();
      double acc[OS_NACC];
#pragma unroll
      for (int k = 0; k < OS_NACC; k++) acc[k] = 0.0;
      for (int i = tid; i < n; i += OS_THREADS) {
        OsPair E;
        if (os_pair(views, pairs, bad, cache, i, E)) continue;
        os_edge(sh_T, K1, E.x2, E.y2, E.z2, E.u1, E.v1, E.w1, delta, sh_J + tid, acc);                    // e12
        os_edge(sh_T + OS_NTRANSFORMS, K2, E.x1, E.y1, E.z1, E.u2, E.v2, E.w2, delta, sh_J + tid, acc);   // e21
      }
      lm_reduce<OS_NACC, OS_NACC, OS_WAVES>(acc, red, Hb, tid);
      double current_chi = Hb[lm_chi<7>];
      if (it == 0) {
        lm.lambda = lm_lambda_init<7>(Hb);
        lm.ni = 2.0;
      }
      double rho = 0.0;
      int qmax = 0;
      do {
        if (tid < 64) {   // the 7 x 7 solve, oplus and the inverse: one wave
          double xs[7];
          const bool ok = lm_ldlt_solve<7>(Hb, lm.lambda, Hb + lm_b<7>, xs);
          OsSim3 t = S;
          if (ok) t = os_oplus(S, xs, fix_scale);
          const OsSim3 ti = os_inverse(t);
          if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 7; j++) sh_x[j] = xs[j];
            sh_trial[0] = t;
            sh_trial[1] = ti;
            sh_ok = ok ? 1 : 0;
          }
        }
        __syncthreads();
        double x[7];
#pragma unroll
        for (int j = 0; j < 7; j++) x[j] = sh_x[j];
        const OsSim3 trial = sh_trial[0], trial_inv = sh_trial[1];
        const bool ok2 = sh_ok != 0;
        __syncthreads();   // read before the next trial's solve writes them again
        double temp_chi = 0.0;
        if (ok2) {   // uniform
          for (int i = tid; i < n; i += OS_THREADS) {
            OsPair E;
            if (os_pair(views, pairs, bad, cache, i, E)) continue;
            double rho0, rho1;
            lm_huber(os_edge_chi2(trial, K1, E.x2, E.y2, E.z2, E.u1, E.v1, E.w1), delta, &rho0, &rho1);
            temp_chi += rho0;
            lm_huber(os_edge_chi2(trial_inv, K2, E.x1, E.y1, E.z1, E.u2, E.v2, E.w2), delta, &rho0, &rho1);
            temp_chi += rho0;
          }
          lm_reduce<1, OS_NACC, OS_WAVES>(&temp_chi, red, &chi_t, tid);
          temp_chi = chi_t;
        }
        if (lm_trial<7>(lm, ok2, current_chi, temp_chi, x, Hb + lm_b<7>, &rho)) {
          current_chi = temp_chi;
          S = trial;
        } else if (!isfinite(lm.lambda)) {
          break;
        }
        qmax++;
      } while (rho < 0 && qmax < 10);
      its++;
      if (qmax == 10 || rho == 0 || !isfinite(lm.lambda)) break;   // Terminate
    }
    if (call == 0)   // not res.iterations[call]: a record indexed at run time would not stay in registers
      res.iterations[0] = its;
    else
      res.iterations[1] = its;
    // Optimizer.cc:1520-1537, :1553-1565 at the call's final estimate
    const OsSim3 Sinv = os_inverse(S);
    int nb = 0;
    for (int i = tid; i < n; i += OS_THREADS) {
      OsPair E;
      if (os_pair(views, pairs, bad, cache, i, E)) continue;
      const double c12 = os_edge_chi2(S, K1, E.x2, E.y2, E.z2, E.u1, E.v1, E.w1);
      const double c21 = os_edge_chi2(Sinv, K2, E.x1, E.y1, E.z1, E.u2, E.v2, E.w2);
      if (c12 > th2 || c21 > th2) {
        bad[i] = 1;
        if (i < OS_LDS_ROWS) cache.flags[i] = 1;
        nb++;
      }
    }
    nb = lm_reduce_count<OS_WAVES>(nb, red_i, tid);
    if (call == 0) {
      n_bad = nb;
      res.n_bad = nb;
      if (n - nb < 10) {   // :1545: return 0, g2oS12 is not written
        if (tid == 0) L.result[p] = res;
        return;
      }
    } else {
      res.n_inliers = n - n_bad - nb;
    }
  }
  if (tid == 0) {
    float v[13];
    os_to_floats(S, v);
    os_set_transform(res, v);
    L.result[p] = res;
  }
}

void orbfe_launch_optimize_sim3(const OsLaunch& L, int P, hipStream_t s) {
  if (P < 1) return;
  hipLaunchKernelGGL(optimize_sim3_kernel, dim3(P), dim3(OS_THREADS), 0, s, L);
}
