// jacobi_internal.h -- the Jacobi arithmetic of every back end that decomposes a small matrix, once.  __host__ __device__ inline
// functions, all in double, compiled with -ffp-contract=off on both sides: THE PARENTHESISATION AND THE SUMMATION ORDER HERE ARE THE
// RESULT.  Nothing of this restates a library routine bit for bit; each caller says which one it stands in for.
//
// Callers:
//   mapping_internal.h      tri_rotate / tri_null_vector: the one-sided form on the named scalars of Triangulate's 4x4; it takes the
//                           rule, the test and the cap from here and writes its own first-minimum pick out (a second copy of
//                           jacobi_first_min's rule: keep the two alike)
//   initializer_internal.h  ini_rot3 / ini_svd3: the same on a 3x3; ini_null9_wave / ini_null9_host: the nine-column null vector in
//                           the initialiser's own lane layout, its column by jacobi_first_min
//   sim3_internal.h         sim3_rotate / sim3_top_eigenvector: the two-sided form on named scalars (app -= t * apq, which is not the
//                           arithmetic of the in-memory update), its column by jacobi_first_max
//   pnp_internal.h          the 3x3 PCA (jacobi_twosided_mem); CC^-1, the 6xk least squares, ABt (jacobi_onesided_mem);
//                           pnp_jacobi12: the round-robin over lanes and LDS
//   optsim3_internal.h and egraph_internal.h reach it through sim3_internal.h, mappoint_internal.h through mapping_internal.h.
// Every caller takes the rotation rule, its convergence test and the sweep cap from here.  The two thresholds are the callers': 2^-50
// in the triangulation and the initialiser, 2^-53 in Sim3 and PnP.  They are not the same number and a result bit hangs on each.
// The register sweeps of the 4x4 and the 3x3 stay with their callers, every element a named scalar: written once here as a template
// over arrays with unrolled loops they give the same bits but another kernel (more registers in triangulate_matches_kernel, one
// wave less per SIMD), and this header changes no listing.
// Non-finite values: both tests are written `!(x > y)`, so a NaN means "do not rotate", and every sweep loop has the cap; nothing can
// loop or trap on a NaN.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define JACOBI_HD __host__ __device__ __forceinline__   // a call that is not inlined would pass the matrices through memory
constexpr int JACOBI_SWEEPS = 30;   // cap; a 3x3 or 4x4 converges in 3-7 sweeps, the nine columns in 6-9, the 12x12 in 8-12

// The rotation rule: t = tan, c = cos, s = sin of the rotation that annihilates the coupling g of two entries a, b -- a_pp, a_qq and
// a_pq of the two-sided form, the squared norms and the dot product of two columns of the one-sided form
JACOBI_HD void jacobi_rotation(double a, double b, double g, double& t, double& c, double& s) {
  const double zeta = (b - a) / (2.0 * g);
  t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  c = 1.0 / sqrt(1.0 + t * t);
  s = c * t;
}
// one-sided: two columns with squared norms alpha, beta and dot product gamma are orthogonal to working precision (also gamma == 0, nan)
JACOBI_HD bool jacobi_orthogonal(double alpha, double beta, double gamma, double eps) { return !(fabs(gamma) > eps * sqrt(alpha * beta)); }
// two-sided: the (p, q) plane of a symmetric matrix is diagonal to working precision (also apq == 0, nan)
JACOBI_HD bool jacobi_diagonal(double app, double aqq, double apq, double eps) { return !(fabs(apq) > eps * (fabs(app) + fabs(aqq))); }

// test and rule of the one-sided form in one: false when the two columns are orthogonal already, else c and s of their rotation
JACOBI_HD bool jacobi_onesided_rotation(double alpha, double beta, double gamma, double eps, double& c, double& s) {
  if (jacobi_orthogonal(alpha, beta, gamma, eps)) return false;
  double t;
  jacobi_rotation(alpha, beta, gamma, t, c, s);
  return true;
}

// The first smallest / the first largest of N values as 0 / 1 weights.  A column taken as the sum of the columns times these weights
// is exact (the entries are finite, one weight is 1) and needs neither selects nor an index: nothing of a matrix held in registers
// may live in scratch memory.  (j and m are declared in the order that keeps each caller's listing; tri_null_vector writes its four
// comparisons out for the same reason.)
template <int N>
JACOBI_HD void jacobi_first_min(const double (&x)[N], double (&s)[N]) {
  int j = 0;
  double m = x[0];
#pragma unroll
  for (int k = 1; k < N; k++)
    if (x[k] < m) { m = x[k]; j = k; }
#pragma unroll
  for (int k = 0; k < N; k++) s[k] = j == k ? 1.0 : 0.0;
}
template <int N>
JACOBI_HD void jacobi_first_max(const double (&x)[N], double (&s)[N]) {
  double m = x[0];
  int j = 0;
#pragma unroll
  for (int k = 1; k < N; k++)
    if (x[k] > m) { m = x[k]; j = k; }
#pragma unroll
  for (int k = 0; k < N; k++) s[k] = j == k ? 1.0 : 0.0;
}

// The one-sided form in memory, one lane: on return the k columns of W (m x k, row-major) are orthogonal and A = W V^T
JACOBI_HD void jacobi_onesided_mem(double* W, double* V, int m, int k, double eps, int sweeps) {
  for (int i = 0; i < k * k; i++) V[i] = (i / k == i % k) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < sweeps; sweep++) {
    bool rotated = false;
    for (int p = 0; p < k - 1; p++)
      for (int q = p + 1; q < k; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int r = 0; r < m; r++) {
          const double x = W[r * k + p], y = W[r * k + q];
          alpha += x * x; beta += y * y; gamma += x * y;
        }
        if (jacobi_orthogonal(alpha, beta, gamma, eps)) continue;
        double t, c, s;
        jacobi_rotation(alpha, beta, gamma, t, c, s);
        for (int r = 0; r < m; r++) {
          const double x = W[r * k + p], y = W[r * k + q];
          W[r * k + p] = c * x - s * y; W[r * k + q] = s * x + c * y;
        }
        for (int r = 0; r < k; r++) {
          const double x = V[r * k + p], y = V[r * k + q];
          V[r * k + p] = c * x - s * y; V[r * k + q] = s * x + c * y;
        }
        rotated = true;
      }
    if (!rotated) break;
  }
}

// The cyclic two-sided form on a symmetric n x n in memory, one lane; V (n x n) receives the eigenvectors in its columns.  Both
// sides of A are rotated with c and s; the register form of sim3_internal.h updates the diagonal with t instead.
JACOBI_HD void jacobi_twosided_mem(double* A, double* V, int n, double eps, int sweeps) {
  for (int i = 0; i < n * n; i++) V[i] = (i / n == i % n) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < sweeps; sweep++) {
    bool rotated = false;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = A[p * n + q], app = A[p * n + p], aqq = A[q * n + q];
        if (jacobi_diagonal(app, aqq, apq, eps)) continue;
        double t, c, s;
        jacobi_rotation(app, aqq, apq, t, c, s);
        for (int k = 0; k < n; k++) {
          double x = A[k * n + p], y = A[k * n + q];
          A[k * n + p] = c * x - s * y; A[k * n + q] = s * x + c * y;
          x = V[k * n + p]; y = V[k * n + q];
          V[k * n + p] = c * x - s * y; V[k * n + q] = s * x + c * y;
        }
        for (int k = 0; k < n; k++) {
          const double x = A[p * n + k], y = A[q * n + k];
          A[p * n + k] = c * x - s * y; A[q * n + k] = s * x + c * y;
        }
        A[p * n + q] = 0.0; A[q * n + p] = 0.0;
        rotated = true;
      }
    if (!rotated) break;
  }
}
