// lm_internal.h -- the generic half of g2o's Levenberg optimiser, once, for every back end: with ONE vertex of N dimensions (N = 6:
// the pose of pose_internal.h, N = 7: the similarity of optsim3_internal.h) and, where stated, for the many vertices of lba_internal.h.  __host__ __device__ inline functions,
// all in double, compiled with -ffp-contract=off on both sides: the parenthesisation of an expression here is its result.  The
// iteration and trial loop itself is not here: what a kernel hands its lanes between solve and trial differs per back end.
//
// Reference (G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o/):
//   RobustKernelHuber::robustify           G/core/robust_kernel_impl.cpp:60-74
//   quadratic form                         G/core/base_fixed_sized_edge.hpp:49-63, :114-130; G/core/base_edge.h:156-162
//   OptimizationAlgorithmLevenberg::solve  G/core/optimization_algorithm_levenberg.cpp:60-176
//   LinearSolverDense::solve               G/solvers/dense/linear_solver_dense.h:96-104
// The dense solver is an unpivoted L D L^T (Eigen::LDLT pivots on the largest diagonal; both report failure on a non-positive
// pivot).  A reading, unpinned.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// The accumulator of one iteration: the N (N + 1) / 2 upper entries of H (row-major, i <= j), then the N of b, then chi
constexpr int lm_H = 0;
template <int N>
constexpr int lm_b = N * (N + 1) / 2;
template <int N>
constexpr int lm_chi = lm_b<N> + N;
template <int N>
constexpr int lm_nacc = lm_chi<N> + 1;

// index of H[i][i] among the upper entries
template <int N>
__host__ __device__ constexpr int lm_diag(int i) {
  return i * N - i * (i - 1) / 2;
}

// RobustKernelHuber::robustify: rho[0] and rho[1]
__host__ __device__ inline void lm_huber(double e, double delta, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  if (e <= dsqr) {
    *rho0 = e;
    *rho1 = 1.0;
  } else {
    const double sqrte = sqrt(e);
    *rho0 = 2 * sqrte * delta - dsqr;
    *rho1 = delta / sqrte;
  }
}

// constructQuadraticForm of one edge with information w * I into acc[lm_nacc<N>]: the Jacobian's rows J0, J1 and -- under `third` --
// J2, the error e0, e1 and e2.  An edge of two rows passes false, any readable row as J2 and any e2: their terms are computed, never
// added, and fold away.  rho1 = 1 without a robust kernel, rho0 = chi2 then.
template <int N>
__host__ __device__ inline void lm_accumulate(const double* J0, const double* J1, const double* J2, bool third, double e0, double e1,
                                              double e2, double w, double rho0, double rho1, double* acc) {
  const double ow = rho1 * w;                            // robustInformation = rho[1] * information
  const double we0 = (-(w * e0)) * rho1;                 // omega_r = -information * error; omega_r *= rho[1]
  const double we1 = (-(w * e1)) * rho1;
  const double we2 = (-(w * e2)) * rho1;
  int k = lm_H;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const double a0 = J0[i] * ow, a1 = J1[i] * ow, a2 = J2[i] * ow;   // A^T * omega
#pragma unroll
    for (int j = i; j < N; j++, k++) {
      double h = a0 * J0[j] + a1 * J1[j];
      if (third) h = h + a2 * J2[j];
      acc[k] += h;
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) {
    double g = J0[i] * we0 + J1[i] * we1;
    if (third) g = g + J2[i] * we2;
    acc[lm_b<N> + i] += g;
  }
  acc[lm_chi<N>] += rho0;
}

// computeLambdaInit: tau * max |H_jj|
template <int N>
__host__ __device__ inline double lm_lambda_init(const double* Hu) {
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < N; i++) m = fmax(fabs(Hu[lm_diag<N>(i)]), m);
  return 1e-5 * m;
}

// (H + lambda I) x = b with H given by its upper entries; false when a pivot is not > 0.  Fully unrolled, no run-time index: a
// matrix indexed at run time lives in scratch memory (DESIGN lesson 58).
template <int N>
__host__ __device__ inline bool lm_ldlt_solve(const double* Hu, double lambda, const double* b, double* x) {
  double H[N][N], L[N][N], D[N], y[N];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int j = i; j < N; j++, k++) {
        H[i][j] = Hu[k];
        H[j][i] = Hu[k];
      }
  }
#pragma unroll
  for (int j = 0; j < N; j++) H[j][j] = H[j][j] + lambda;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; j++) {
    double d = H[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * D[k];
    if (!(d > 0.0)) ok = false;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      double s = H[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k] * D[k];
      L[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
    y[i] = s;
  }
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    double s = y[i] / D[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) s -= L[k][i] * x[k];
    x[i] = s;
  }
  return ok;
}

// The state of OptimizationAlgorithmLevenberg across the iterations of one optimize() call
struct LmState {
  double lambda, ni;
};

// Good / bad step bookkeeping of one trial (optimization_algorithm_levenberg.cpp:125-146) with computeScale's sum over the update
// vector handed in: the form for a system of many vertices (lba_internal.h), whose x and b are no fixed-size arrays.  `scale_sum` is
// read only when ok2.  Returns true when the step is accepted.
__host__ __device__ inline bool lm_trial_scaled(LmState& lm, bool ok2, double current_chi, double temp_chi, double scale_sum,
                                                double* rho_out) {
  double scale = 1.0;
  if (ok2) {
    scale = scale_sum + 1e-3;
  } else {
    temp_chi = 1.7976931348623157e308;   // std::numeric_limits<double>::max()
  }
  const double rho = (current_chi - temp_chi) / scale;
  *rho_out = rho;
  if (rho > 0 && isfinite(temp_chi) && ok2) {
    const double c = 2 * rho - 1;
    double alpha = 1. - c * c * c;       // pow(2 rho - 1, 3)
    alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
    const double f = 1. / 3. < alpha ? alpha : 1. / 3.;
    lm.lambda *= f;
    lm.ni = 2;
    return true;
  }
  lm.lambda *= lm.ni;
  lm.ni *= 2;
  return false;
}

// The same for ONE vertex of N dimensions: computeScale over its x and b
template <int N>
__host__ __device__ inline bool lm_trial(LmState& lm, bool ok2, double current_chi, double temp_chi, const double* x, const double* b,
                                         double* rho_out) {
  double scale = 0.0;
  if (ok2) {
#pragma unroll
    for (int j = 0; j < N; j++) scale += x[j] * (lm.lambda * x[j] + b[j]);   // computeScale
  }
  return lm_trial_scaled(lm, ok2, current_chi, temp_chi, scale, rho_out);
}
