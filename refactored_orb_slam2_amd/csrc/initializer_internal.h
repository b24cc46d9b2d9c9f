// initializer_internal.h -- the arithmetic of Initializer::Initialize, once, for the kernels (initializer_kernels.hip) and for host
// code that wants the same bits (tests/cpp_initializer/host_arith.cpp).  __host__ __device__ inline functions, compiled with
// -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   Normalize                              L/src/Initializer.cc:739-783
//   ComputeH21 / ComputeF21                L/src/Initializer.cc:218-292
//   FindHomography / FindFundamental       L/src/Initializer.cc:124-216 (the products around the solver, the selection)
//   CheckHomography / CheckFundamental     L/src/Initializer.cc:294-459
//   ReconstructF / DecomposeE              L/src/Initializer.cc:461-560, :901-921
//   ReconstructH                           L/src/Initializer.cc:562-721
//   Triangulate / CheckRT                  L/src/Initializer.cc:723-737, :785-899
// cv::Mat arithmetic is read as mapping_internal.h and sim3_internal.h read it: a matrix product is a float dot product per
// element in index order (zeros of a sparse factor included: x * 0 + y is y for finite x), a gemm with a scalar folded in multiplies
// the float dot by the scalar in double, a gemm with an addend adds it in double, Mat::dot and cv::norm accumulate in double in
// element order, `Mat / scalar` multiplies by (float)(1.0 / scalar).  `1.0 / x` assigned to a float divides in double.
// What is not available where this library is built is stated here; the rotation rule, its convergence test, the
// sweep cap and the column pick of both decompositions are jacobi_internal.h's:
//   cv::SVDecomp of the 16x9 / 8x9   ini_null9_*: one-sided (Hestenes) Jacobi in double on the float entries; a lane -- or, on the
//                                    host, an array element -- holds one ROW of [A; V] as nine named doubles, the 36 column pairs of
//                                    a sweep are written out, the three dot products of a pair are sums over the 16 rows of A in the
//                                    order of a 16-lane xor butterfly (8, 4, 2, 1).  vt.row(8) is the column of V that belongs to the
//                                    smallest column norm, rounded to float.
//   cv::SVDecomp / cv::SVD::compute of a 3x3   ini_svd3: the same method on named scalars; singular values descending, u0 and u1 the
//                                    normalised columns of A V, u2 = +-(u0 x u1) with the sign of its projection on the third column,
//                                    which is orthonormal also where the third singular value is 0 (the essential matrix)
//   cv::Mat::inv, cv::determinant of a 3x3     the cofactor forms in double of OpenCV's own small-matrix paths; inv of a singular
//                                    matrix is the zero matrix
// The sign of a null vector changes no output: CheckHomography uses ratios, CheckFundamental squares, ReconstructH ratios of
// singular values, s = det U * det Vt and a normalised t, ReconstructF both signs of t and a determinant test.  It is fixed (the entry
// of largest magnitude, the first among equals, is positive) so that bytes are deterministic.  The signs of the 3x3 vectors decide
// the ORDER of the motion candidates, never their set.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <stdint.h>

#include "../../include/orbfe.h"
#include "mapping_internal.h"   // tri_null_vector: the 4x4 of Triangulate

#define INI_HD __host__ __device__ __forceinline__
#define INI_JACOBI_EPS 0x1p-50  // "orthogonal to working precision" of float entries; the 9 columns converge in 6-9 sweeps, a 3x3 in 3-5
#define INI_WAVES 4            // hypotheses (waves) per workgroup of initz_hypotheses_kernel
#define INI_RT_THREADS 256     // of a CheckRT workgroup

// ---- 3x3 helpers, row-major
INI_HD void ini_mul33(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
INI_HD void ini_transpose33(const float* A, float* T) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}
// cv::determinant of a float 3x3: det3 in double
INI_HD double ini_det33(const float* m) {
  return (double)m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - (double)m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
         (double)m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}
// cv::Mat::inv of a float 3x3 (DECOMP_LU takes the closed form for n <= 3): cofactors in double times 1 / det, rounded once
INI_HD void ini_inv33(const float* m, float* o) {
  double d = ini_det33(m);
  if (d == 0.0) {
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = 0.0f;
    return;
  }
  d = 1.0 / d;
  o[0] = (float)(((double)m[4] * m[8] - (double)m[5] * m[7]) * d);
  o[1] = (float)(((double)m[2] * m[7] - (double)m[1] * m[8]) * d);
  o[2] = (float)(((double)m[1] * m[5] - (double)m[2] * m[4]) * d);
  o[3] = (float)(((double)m[5] * m[6] - (double)m[3] * m[8]) * d);
  o[4] = (float)(((double)m[0] * m[8] - (double)m[2] * m[6]) * d);
  o[5] = (float)(((double)m[2] * m[3] - (double)m[0] * m[5]) * d);
  o[6] = (float)(((double)m[3] * m[7] - (double)m[4] * m[6]) * d);
  o[7] = (float)(((double)m[1] * m[6] - (double)m[0] * m[7]) * d);
  o[8] = (float)(((double)m[0] * m[4] - (double)m[1] * m[3]) * d);
}
INI_HD void ini_K(const orbfe_init_params& p, float* K) {
  K[0] = p.fx; K[1] = 0; K[2] = p.cx; K[3] = 0; K[4] = p.fy; K[5] = p.cy; K[6] = 0; K[7] = 0; K[8] = 1;
}

// ---- Normalize (:739-783): float sums in index order over all n keypoints, never reassociated.  The x and the y sums do not meet,
// so one call handles one coordinate (v[0], v[stride], ...): its mean and its scale 1 / meanDev
struct IniNorm { float mx, my, sx, sy; };
INI_HD void ini_normalize_coordinate(const float* v, int stride, int n, float& mean_out, float& scale_out) {
  float mean = 0;
  for (int i = 0; i < n; i++) mean += v[(size_t)i * stride];
  mean = mean / n;
  float meanDev = 0;
  for (int i = 0; i < n; i++) meanDev += fabsf(v[(size_t)i * stride] - mean);
  meanDev = meanDev / n;
  mean_out = mean;
  scale_out = (float)(1.0 / (double)meanDev);
}
INI_HD void ini_normalize(const float* keys, int n, IniNorm& N) {
  ini_normalize_coordinate(keys, 2, n, N.mx, N.sx);
  ini_normalize_coordinate(keys + 1, 2, n, N.my, N.sy);
}
INI_HD void ini_norm_matrix(const IniNorm& N, float* T) {   // :778-782
  T[0] = N.sx; T[1] = 0; T[2] = -N.mx * N.sx; T[3] = 0; T[4] = N.sy; T[5] = -N.my * N.sy; T[6] = 0; T[7] = 0; T[8] = 1;
}
INI_HD float ini_norm_x(const IniNorm& N, float x) { return (x - N.mx) * N.sx; }   // :760, :774
INI_HD float ini_norm_y(const IniNorm& N, float y) { return (y - N.my) * N.sy; }

// ---- the 9-column null vector
struct IniRow { double c0, c1, c2, c3, c4, c5, c6, c7, c8; };   // one row of [A; V]

// row 2 i (odd = false) or 2 i + 1 (odd = true) of ComputeH21's A (:230-248): float entries, widened
INI_HD IniRow ini_row_h(bool odd, float u1, float v1, float u2, float v2) {
  IniRow r;
  if (!odd) {
    r.c0 = 0.0; r.c1 = 0.0; r.c2 = 0.0; r.c3 = (double)-u1; r.c4 = (double)-v1; r.c5 = -1.0;
    r.c6 = (double)(v2 * u1); r.c7 = (double)(v2 * v1); r.c8 = (double)v2;
  } else {
    r.c0 = (double)u1; r.c1 = (double)v1; r.c2 = 1.0; r.c3 = 0.0; r.c4 = 0.0; r.c5 = 0.0;
    r.c6 = (double)(-u2 * u1); r.c7 = (double)(-u2 * v1); r.c8 = (double)-u2;
  }
  return r;
}
// row i of ComputeF21's A (:270-278)
INI_HD IniRow ini_row_f(float u1, float v1, float u2, float v2) {
  IniRow r;
  r.c0 = (double)(u2 * u1); r.c1 = (double)(u2 * v1); r.c2 = (double)u2; r.c3 = (double)(v2 * u1); r.c4 = (double)(v2 * v1);
  r.c5 = (double)v2; r.c6 = (double)u1; r.c7 = (double)v1; r.c8 = 1.0;
  return r;
}
// row k of the identity (k outside 0 .. 8: a zero row)
INI_HD IniRow ini_row_v(int k) {
  IniRow r;
  r.c0 = k == 0; r.c1 = k == 1; r.c2 = k == 2; r.c3 = k == 3; r.c4 = k == 4; r.c5 = k == 5; r.c6 = k == 6; r.c7 = k == 7; r.c8 = k == 8;
  return r;
}
// the 36 pairs of a cyclic sweep, every index a literal
#define INI_SWEEP(P)                                                                                                          \
  P(0, 1) P(0, 2) P(0, 3) P(0, 4) P(0, 5) P(0, 6) P(0, 7) P(0, 8) P(1, 2) P(1, 3) P(1, 4) P(1, 5) P(1, 6) P(1, 7) P(1, 8) P(2, 3) \
  P(2, 4) P(2, 5) P(2, 6) P(2, 7) P(2, 8) P(3, 4) P(3, 5) P(3, 6) P(3, 7) P(3, 8) P(4, 5) P(4, 6) P(4, 7) P(4, 8) P(5, 6) P(5, 7)   \
  P(5, 8) P(6, 7) P(6, 8) P(7, 8)
#define INI_COLUMNS(C) C(0) C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(8)
// the sign convention: the entry of largest magnitude, the first among equals, becomes positive; then the rounding to float
INI_HD void ini_null9_finish(const double* w, float* v) {
  double m = -1.0, sg = 1.0;
#pragma unroll
  for (int k = 0; k < 9; k++)
    if (fabs(w[k]) > m) { m = fabs(w[k]); sg = w[k] < 0.0 ? -1.0 : 1.0; }
#pragma unroll
  for (int k = 0; k < 9; k++) v[k] = (float)(w[k] * sg);
}

#if defined(__HIP__)   // the translation unit is HIP: a kernel file
__device__ __forceinline__ double ini_uniform_d(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
// the sum over lanes 0 .. 15 in butterfly order, the same value in every lane of the wave
__device__ __forceinline__ double ini_sum16(double x) {
  x += __shfl_xor(x, 8);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 1);
  return ini_uniform_d(x);
}
// The wave form: lane l < 16 holds row l of A (zero rows behind the model's own), lane 16 + k row k of V = I, every other lane a
// zero row.  All 64 lanes call it; v[9] is wave-uniform.
__device__ __forceinline__ void ini_null9_wave(IniRow r, int lane, float* v) {
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
    bool rotated = false;
#define INI_PAIR(p, q)                                                                                                       \
  {                                                                                                                          \
    const double alpha = ini_sum16(r.c##p * r.c##p), beta = ini_sum16(r.c##q * r.c##q), gamma = ini_sum16(r.c##p * r.c##q); \
    double c, s;                                                                                                             \
    if (jacobi_onesided_rotation(alpha, beta, gamma, INI_JACOBI_EPS, c, s)) {                                                \
      rotated = true;                                                                                                        \
      const double x = r.c##p;                                                                                               \
      r.c##p = c * x - s * r.c##q;                                                                                           \
      r.c##q = s * x + c * r.c##q;                                                                                           \
    }                                                                                                                        \
  }
    INI_SWEEP(INI_PAIR)
#undef INI_PAIR
    if (!rotated) break;   // uniform: alpha, beta, gamma are
  }
  double n[9], s[9], w[9];
#define INI_NORM(k) n[k] = ini_sum16(r.c##k * r.c##k);
  INI_COLUMNS(INI_NORM)
#undef INI_NORM
  jacobi_first_min(n, s);
  double mine = 0.0;
#define INI_TAKE(k) mine += r.c##k * s[k];
  INI_COLUMNS(INI_TAKE)
#undef INI_TAKE
#pragma unroll
  for (int k = 0; k < 9; k++) w[k] = __shfl(mine, 16 + k);
  ini_null9_finish(w, v);
}
#endif

// The host form of the same arithmetic: rows[0 .. 16) of A, rows[16 .. 25) of V = I
inline double ini_tree16(const double* x) {
  double y[16], z[16];
  for (int i = 0; i < 16; i++) y[i] = x[i];
  for (int d = 8; d > 0; d >>= 1) {
    for (int i = 0; i < 16; i++) z[i] = y[i] + y[i ^ d];
    for (int i = 0; i < 16; i++) y[i] = z[i];
  }
  return y[0];
}
inline void ini_null9_host(IniRow* rows, float* v) {
  double xa[16], xb[16], xg[16];
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
    bool rotated = false;
#define INI_PAIR(p, q)                                                                   \
  {                                                                                      \
    for (int l = 0; l < 16; l++) {                                                       \
      xa[l] = rows[l].c##p * rows[l].c##p;                                               \
      xb[l] = rows[l].c##q * rows[l].c##q;                                               \
      xg[l] = rows[l].c##p * rows[l].c##q;                                               \
    }                                                                                    \
    const double alpha = ini_tree16(xa), beta = ini_tree16(xb), gamma = ini_tree16(xg);  \
    double c, s;                                                                         \
    if (jacobi_onesided_rotation(alpha, beta, gamma, INI_JACOBI_EPS, c, s)) {            \
      rotated = true;                                                                    \
      for (int l = 0; l < 25; l++) {                                                     \
        const double x = rows[l].c##p;                                                   \
        rows[l].c##p = c * x - s * rows[l].c##q;                                         \
        rows[l].c##q = s * x + c * rows[l].c##q;                                         \
      }                                                                                  \
    }                                                                                    \
  }
    INI_SWEEP(INI_PAIR)
#undef INI_PAIR
    if (!rotated) break;
  }
  double n[9], s[9], w[9];
#define INI_NORM(k)                                                       \
  for (int l = 0; l < 16; l++) xa[l] = rows[l].c##k * rows[l].c##k;       \
  n[k] = ini_tree16(xa);
  INI_COLUMNS(INI_NORM)
#undef INI_NORM
  jacobi_first_min(n, s);
  for (int k = 0; k < 9; k++) {
    double mine = 0.0;
#define INI_TAKE(j) mine += rows[16 + k].c##j * s[j];
    INI_COLUMNS(INI_TAKE)
#undef INI_TAKE
    w[k] = mine;
  }
  ini_null9_finish(w, v);
}

// ---- the 3x3 decomposition
INI_HD bool ini_rot3(double& a0p, double& a1p, double& a2p, double& a0q, double& a1q, double& a2q, double& v0p, double& v1p, double& v2p,
                     double& v0q, double& v1q, double& v2q) {
  const double alpha = a0p * a0p + a1p * a1p + a2p * a2p, beta = a0q * a0q + a1q * a1q + a2q * a2q, gamma = a0p * a0q + a1p * a1q + a2p * a2q;
  double c, s;
  if (!jacobi_onesided_rotation(alpha, beta, gamma, INI_JACOBI_EPS, c, s)) return false;
  double x;
  x = a0p; a0p = c * x - s * a0q; a0q = s * x + c * a0q;
  x = a1p; a1p = c * x - s * a1q; a1q = s * x + c * a1q;
  x = a2p; a2p = c * x - s * a2q; a2q = s * x + c * a2q;
  x = v0p; v0p = c * x - s * v0q; v0q = s * x + c * v0q;
  x = v1p; v1p = c * x - s * v1q; v1q = s * x + c * v1q;
  x = v2p; v2p = c * x - s * v2q; v2q = s * x + c * v2q;
  return true;
}
INI_HD void ini_swap_columns(bool swap, double& n0, double& b0, double& b1, double& b2, double& v0, double& v1, double& v2, double& n1,
                             double& c0, double& c1, double& c2, double& w0, double& w1, double& w2) {
  double x;
  x = n0; n0 = swap ? n1 : n0; n1 = swap ? x : n1;
  x = b0; b0 = swap ? c0 : b0; c0 = swap ? x : c0;
  x = b1; b1 = swap ? c1 : b1; c1 = swap ? x : c1;
  x = b2; b2 = swap ? c2 : b2; c2 = swap ? x : c2;
  x = v0; v0 = swap ? w0 : v0; w0 = swap ? x : w0;
  x = v1; v1 = swap ? w1 : v1; w1 = swap ? x : w1;
  x = v2; v2 = swap ? w2 : v2; w2 = swap ? x : w2;
}
// A = U diag(w) Vt of a float 3x3, w descending, all three rounded to float from double
INI_HD void ini_svd3(const float* A, float* U, float* w, float* Vt) {
  double a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[3], a11 = A[4], a12 = A[5], a20 = A[6], a21 = A[7], a22 = A[8];
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
    bool rotated = false;
    rotated |= ini_rot3(a00, a10, a20, a01, a11, a21, v00, v10, v20, v01, v11, v21);   // (0, 1)
    rotated |= ini_rot3(a00, a10, a20, a02, a12, a22, v00, v10, v20, v02, v12, v22);   // (0, 2)
    rotated |= ini_rot3(a01, a11, a21, a02, a12, a22, v01, v11, v21, v02, v12, v22);   // (1, 2)
    if (!rotated) break;
  }
  double n0 = a00 * a00 + a10 * a10 + a20 * a20, n1 = a01 * a01 + a11 * a11 + a21 * a21, n2 = a02 * a02 + a12 * a12 + a22 * a22;
  // descending, stable: three compare-exchanges of whole columns
  ini_swap_columns(n0 < n1, n0, a00, a10, a20, v00, v10, v20, n1, a01, a11, a21, v01, v11, v21);
  ini_swap_columns(n1 < n2, n1, a01, a11, a21, v01, v11, v21, n2, a02, a12, a22, v02, v12, v22);
  ini_swap_columns(n0 < n1, n0, a00, a10, a20, v00, v10, v20, n1, a01, a11, a21, v01, v11, v21);
  const double s0 = sqrt(n0), s1 = sqrt(n1), s2 = sqrt(n2);
  const double i0 = 1.0 / s0, i1 = 1.0 / s1;
  const double u00 = a00 * i0, u10 = a10 * i0, u20 = a20 * i0, u01 = a01 * i1, u11 = a11 * i1, u21 = a21 * i1;
  double u02 = u10 * u21 - u20 * u11, u12 = u20 * u01 - u00 * u21, u22 = u00 * u11 - u10 * u01;
  const double sg = (u02 * a02 + u12 * a12 + u22 * a22) < 0.0 ? -1.0 : 1.0;
  u02 *= sg; u12 *= sg; u22 *= sg;
  U[0] = (float)u00; U[1] = (float)u01; U[2] = (float)u02; U[3] = (float)u10; U[4] = (float)u11; U[5] = (float)u12;
  U[6] = (float)u20; U[7] = (float)u21; U[8] = (float)u22;
  w[0] = (float)s0; w[1] = (float)s1; w[2] = (float)s2;
  Vt[0] = (float)v00; Vt[1] = (float)v10; Vt[2] = (float)v20; Vt[3] = (float)v01; Vt[4] = (float)v11; Vt[5] = (float)v21;
  Vt[6] = (float)v02; Vt[7] = (float)v12; Vt[8] = (float)v22;
}

// ---- the two models behind the null vector
// FindHomography :157-159: H21i = T2inv * Hn * T1, H12i = H21i.inv()
INI_HD void ini_model_h(const float* Hn, const float* T1, const float* T2inv, float* H21, float* H12) {
  float tmp[9];
  ini_mul33(T2inv, Hn, tmp);
  ini_mul33(tmp, T1, H21);
  ini_inv33(H21, H12);
}
// ComputeF21 :285-291 and FindFundamental :206: the rank-2 step, then F21i = T2t * Fn * T1
INI_HD void ini_model_f(const float* Fpre, const float* T1, const float* T2t, float* F21) {
  float U[9], w[3], Vt[9], uw[9], Fn[9], tmp[9];
  ini_svd3(Fpre, U, w, Vt);
  w[2] = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) uw[3 * i + j] = U[3 * i + j] * w[j];
  ini_mul33(uw, Vt, Fn);
  ini_mul33(T2t, Fn, tmp);
  ini_mul33(tmp, T1, F21);
}

// ---- the per-match tests; `add` is what the match adds to the score, first term first
INI_HD float ini_inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }
// CheckHomography :327-376
INI_HD bool ini_check_h(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float invSigmaSquare, float& add1,
                        float& add2) {
  const float th = 5.991f;
  bool bIn = true;
  add1 = 0.0f; add2 = 0.0f;
  const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
  const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
  const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
  const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false;
  else add1 = th - chiSquare1;
  const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
  const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
  const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
  const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false;
  else add2 = th - chiSquare2;
  return bIn;
}
// CheckFundamental :405-456
INI_HD bool ini_check_f(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare, float& add1, float& add2) {
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  add1 = 0.0f; add2 = 0.0f;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false;
  else add1 = thScore - chiSquare1;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false;
  else add2 = thScore - chiSquare2;
  return bIn;
}
// true when the eight indices can be a draw of :80-93: inside [0, N) and pairwise different
INI_HD bool ini_set_ok(const int32_t* s, int N) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 8; a++) {
    ok = ok && s[a] >= 0 && s[a] < N;
#pragma unroll
    for (int b = 0; b < a; b++) ok = ok && s[a] != s[b];
  }
  return ok;
}
// `currentScore > score` from score = 0 (:163, :210): hypothesis h with score sc replaces (best, best_score) when it is better, or
// equal and earlier -- the order-free statement of "the first maximum"; a zero or NaN score never wins
INI_HD void ini_first_max(float sc, int h, float& best_score, int& best) {
  if (sc > 0.0f && (sc > best_score || (sc == best_score && best >= 0 && h < best))) {
    best_score = sc;
    best = h;
  }
}

// ---- the motion candidates
// DecomposeE (:901-921) behind E21 = K.t() * F21 * K (:472); candidates in the order of :488-495: (R1, t), (R2, t), (R1, -t), (R2, -t)
INI_HD void ini_candidates_f(const float* F21, const float* K, orbfe_init_candidate* out) {
  float Kt[9], tmp[9], E[9], U[9], w[3], Vt[9];
  ini_transpose33(K, Kt);
  ini_mul33(Kt, F21, tmp);
  ini_mul33(tmp, K, E);
  ini_svd3(E, U, w, Vt);
  float t[3] = {U[2], U[5], U[8]};
  const float inv = (float)(1.0 / tri_norm3(t));
  t[0] *= inv; t[1] *= inv; t[2] *= inv;
  const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
  float R1[9], R2[9];
  ini_mul33(U, W, tmp);
  ini_mul33(tmp, Vt, R1);
  if (ini_det33(R1) < 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) R1[k] = -R1[k];
  }
  ini_mul33(U, Wt, tmp);
  ini_mul33(tmp, Vt, R2);
  if (ini_det33(R2) < 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) R2[k] = -R2[k];
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
#pragma unroll
    for (int k = 0; k < 9; k++) out[c].R[k] = (c & 1) ? R2[k] : R1[k];
#pragma unroll
    for (int k = 0; k < 3; k++) out[c].t[k] = (c & 2) ? -t[k] : t[k];
    out[c].n_good = 0; out[c].parallax = 0.0f; out[c].reserved[0] = 0; out[c].reserved[1] = 0;
  }
}
// one Faugeras motion: R = s * U * Rp * Vt (:619, :657), t = U * tp / norm (:628-629, :666-667)
INI_HD void ini_faugeras_one(const float* U, const float* Vt, float s, const float* Rp, const float* tp, orbfe_init_candidate& o) {
  float tmp[9];
  ini_mul33(U, Rp, tmp);
#pragma unroll
  for (int k = 0; k < 9; k++) tmp[k] = (float)((double)tmp[k] * (double)s);   // the gemm with the scalar folded in
  ini_mul33(tmp, Vt, o.R);
  float t[3];
#pragma unroll
  for (int r = 0; r < 3; r++) t[r] = U[3 * r] * tp[0] + U[3 * r + 1] * tp[1] + U[3 * r + 2] * tp[2];
  const float inv = (float)(1.0 / tri_norm3(t));
#pragma unroll
  for (int r = 0; r < 3; r++) o.t[r] = t[r] * inv;
  o.n_good = 0; o.parallax = 0.0f; o.reserved[0] = 0; o.reserved[1] = 0;
}
// ReconstructH :577-678.  false: the exit of :590, nothing is written
INI_HD bool ini_candidates_h(const float* H21, const float* K, orbfe_init_candidate* out) {
  float invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
  ini_inv33(K, invK);
  ini_mul33(invK, H21, tmp);
  ini_mul33(tmp, K, A);
  ini_svd3(A, U, w, Vt);
  const float s = (float)(ini_det33(U) * ini_det33(Vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
    const float stheta = (i == 0 || i == 3) ? aux_stheta : -aux_stheta, sphi = (i == 0 || i == 3) ? aux_sphi : -aux_sphi;
    const float Rp1[9] = {ctheta, 0, -stheta, 0, 1, 0, stheta, 0, ctheta};
    const float tp1[3] = {x1 * (d1 - d3), 0 * (d1 - d3), -x3 * (d1 - d3)};
    ini_faugeras_one(U, Vt, s, Rp1, tp1, out[i]);
    const float Rp2[9] = {cphi, 0, sphi, 0, -1, 0, sphi, 0, -cphi};
    const float tp2[3] = {x1 * (d1 + d3), 0 * (d1 + d3), x3 * (d1 + d3)};
    ini_faugeras_one(U, Vt, s, Rp2, tp2, out[4 + i]);
  }
  return true;
}

// ---- CheckRT (:785-899)
struct IniPose { float R[9], t[3], P2[12], O2[3]; };
INI_HD void ini_pose(const float* K, const float* R, const float* t, IniPose& P) {
#pragma unroll
  for (int k = 0; k < 9; k++) P.R[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) P.t[k] = t[k];
#pragma unroll
  for (int r = 0; r < 3; r++) {   // :814  P2 = K * [R | t]
#pragma unroll
    for (int c = 0; c < 3; c++) P.P2[4 * r + c] = K[3 * r] * R[c] + K[3 * r + 1] * R[3 + c] + K[3 * r + 2] * R[6 + c];
    P.P2[4 * r + 3] = K[3 * r] * t[0] + K[3 * r + 1] * t[1] + K[3 * r + 2] * t[2];
    P.O2[r] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);   // :816  O2 = -R.t() * t
  }
}
// the body of the loop :824-887 for one inlier: 0 = rejected, 1 = counted (its cosine is pushed, vP3D set), 2 = counted and vbGood
INI_HD int ini_check_point(const orbfe_init_params& C, const float* K, const IniPose& P, float th2, float x1, float y1, float x2, float y2,
                           float* p, float& cosParallax) {
  // Triangulate (:726-736); P1 = K [I | 0]
  float A[16], v[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const float p10 = c < 3 ? K[c] : 0.0f, p11 = c < 3 ? K[3 + c] : 0.0f, p12 = c < 3 ? K[6 + c] : 0.0f;
    A[c] = x1 * p12 - p10;
    A[4 + c] = y1 * p12 - p11;
    A[8 + c] = x2 * P.P2[8 + c] - P.P2[c];
    A[12 + c] = y2 * P.P2[8 + c] - P.P2[4 + c];
  }
  tri_null_vector(A, v);
  const float inv_w = (float)(1.0 / (double)v[3]);
  p[0] = v[0] * inv_w; p[1] = v[1] * inv_w; p[2] = v[2] * inv_w;
  cosParallax = 0.0f;
  if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) return 0;
  const float n2[3] = {p[0] - P.O2[0], p[1] - P.O2[1], p[2] - P.O2[2]};
  const float dist1 = (float)tri_norm3(p), dist2 = (float)tri_norm3(n2);
  cosParallax = (float)(tri_dot3(p, n2) / (double)(dist1 * dist2));
  if (p[2] <= 0 && (double)cosParallax < 0.99998) return 0;
  float q[3];
#pragma unroll
  for (int r = 0; r < 3; r++) q[r] = (float)((double)(P.R[3 * r] * p[0] + P.R[3 * r + 1] * p[1] + P.R[3 * r + 2] * p[2]) + (double)P.t[r]);
  if (q[2] <= 0 && (double)cosParallax < 0.99998) return 0;
  const float invZ1 = (float)(1.0 / (double)p[2]);
  const float im1x = C.fx * p[0] * invZ1 + C.cx, im1y = C.fy * p[1] * invZ1 + C.cy;
  const float squareError1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
  if (squareError1 > th2) return 0;
  const float invZ2 = (float)(1.0 / (double)q[2]);
  const float im2x = C.fx * q[0] * invZ2 + C.cx, im2y = C.fy * q[1] * invZ2 + C.cy;
  const float squareError2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
  if (squareError2 > th2) return 0;
  return (double)cosParallax < 0.99998 ? 2 : 1;
}
INI_HD float ini_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }   // :489  4.0 * mSigma2 into a float parameter
// a float cosine as an unsigned key of the same order; NaN (undefined in std::sort) sorts last
INI_HD uint32_t ini_cos_key(float c) {
  if (c != c) return 0xfffffffeu;
  uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = __float_as_uint(c);
#else
  memcpy(&b, &c, 4);
#endif
  const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return k > 0xfffffffeu ? 0xfffffffeu : k;
}
INI_HD float ini_key_cos(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float c;
#if defined(__HIP_DEVICE_COMPILE__)
  c = __uint_as_float(b);
#else
  memcpy(&c, &b, 4);
#endif
  return k == 0xfffffffeu ? NAN : c;
}
// :894  acos(cos) * 180 / CV_PI: the float acos (evaluated in double and rounded), a float product, a double quotient
INI_HD float ini_parallax_degrees(float c) {
  const float a = (float)acos((double)c);
  return (float)((double)(a * 180) / 3.1415926535897932384626433832795);
}

// ---- the acceptance rules.  Both fill model-independent fields of r and return success.
// ReconstructF :497-559 over the four (n_good, parallax)
INI_HD bool ini_decide_f(const orbfe_init_candidate* c, int N, const orbfe_init_params& p, orbfe_init_result& r) {
  const int g1 = c[0].n_good, g2 = c[1].n_good, g3 = c[2].n_good, g4 = c[3].n_good;
  const int m34 = g3 > g4 ? g3 : g4, m234 = g2 > m34 ? g2 : m34, maxGood = g1 > m234 ? g1 : m234;
  const int n09 = (int)(0.9 * N), nMinGood = n09 > p.min_triangulated ? n09 : p.min_triangulated;
  int nsimilar = 0;
  if (g1 > 0.7 * maxGood) nsimilar++;
  if (g2 > 0.7 * maxGood) nsimilar++;
  if (g3 > 0.7 * maxGood) nsimilar++;
  if (g4 > 0.7 * maxGood) nsimilar++;
  const int best = maxGood == g1 ? 0 : (maxGood == g2 ? 1 : (maxGood == g3 ? 2 : 3));
  r.best_candidate = best;
  r.n_good = maxGood;
  r.second_good_or_n_similar = nsimilar;
  r.parallax = c[best].parallax;
  int reason = 0;
  if (maxGood < nMinGood) reason |= ORBFE_INIT_F_FEW_GOOD;
  if (nsimilar > 1) reason |= ORBFE_INIT_F_SIMILAR;
  if (!reason && !(c[best].parallax > p.min_parallax)) reason |= ORBFE_INIT_F_PARALLAX;
  r.reason |= reason;
  return reason == 0;
}
// ReconstructH :680-720 over the eight
INI_HD bool ini_decide_h(const orbfe_init_candidate* c, int N, const orbfe_init_params& p, orbfe_init_result& r) {
  int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
  float bestParallax = -1;
  for (int i = 0; i < 8; i++) {
    const int nGood = c[i].n_good;
    if (nGood > bestGood) {
      secondBestGood = bestGood;
      bestGood = nGood;
      bestSolutionIdx = i;
      bestParallax = c[i].parallax;
    } else if (nGood > secondBestGood) {
      secondBestGood = nGood;
    }
  }
  r.best_candidate = bestSolutionIdx;
  r.n_good = bestGood;
  r.second_good_or_n_similar = secondBestGood;
  r.parallax = bestParallax;
  int reason = 0;
  if (!(secondBestGood < 0.75 * bestGood)) reason |= ORBFE_INIT_H_SECOND;
  if (!(bestParallax >= p.min_parallax)) reason |= ORBFE_INIT_H_PARALLAX;
  if (!(bestGood > p.min_triangulated)) reason |= ORBFE_INIT_H_MIN_TRIANGULATED;
  if (!(bestGood > 0.9 * N)) reason |= ORBFE_INIT_H_FEW_GOOD;
  r.reason |= reason;
  return reason == 0;
}

// ---- launchers (initializer_kernels.hip)
struct IniHeader {          // per problem, written by the prologue: 160 bytes
  int32_t N, n1, n2, pad;   // matches, clamped key counts
  IniNorm N1, N2;
  float T1[9], T2inv[9], T2t[9];
  int32_t pad2;
};
struct IniLaunch {
  const orbfe_init_params* params;                                  // [P]
  const float* keys1; const float* keys2;                           // [P][cap][2]
  const int32_t* n1; const int32_t* n2; int cap;                    // [P]
  const int32_t* matches12;                                         // [P][cap]
  const int32_t* sets; const int32_t* H; int h_cap;                 // [P][h_cap][8], [P]
  orbfe_init_result* result;                                        // [P]
  float* P3D; uint64_t* triangulated; uint64_t* inlier_words;       // [P][cap][3], [P][W], [P][W]; W = ceil(cap / 64)
  orbfe_init_hypothesis* hyps; uint64_t* words;                     // [P][2][h_cap], [P][2][h_cap][W]
  orbfe_init_candidate* cands;                                      // [P][8]
  IniHeader* header; float4* mxy; int32_t* mi1;                     // workspace: [P], [P][cap] (u1, v1, u2, v2), [P][cap] index into keys1
};
void orbfe_launch_initializer(const IniLaunch& L, int P, hipStream_t s);
