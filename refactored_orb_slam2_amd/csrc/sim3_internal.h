// sim3_internal.h -- the arithmetic of Sim3Solver, once, for the kernels (sim3_kernels.hip) and for host code that wants the same
// bits.  __host__ __device__ inline functions, compiled with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   the constructor's preparation per kept match    L/src/Sim3Solver.cc:92-96, :376-393 (FromCameraToImage)
//   ComputeCentroid / ComputeSim3                   L/src/Sim3Solver.cc:207-322
//   CheckInliers / Project                          L/src/Sim3Solver.cc:324-344, :354-374
// cv::Mat arithmetic is read as mapping_internal.h reads it: a matrix product is a float dot product per element in index order, a
// `scalar * Mat` held in a float Mat multiplies by (float)scalar, a gemm with a scalar folded in multiplies the float dot by the
// scalar in double, Mat::dot and cv::norm accumulate in double in element order.  What the file keeps in double stays double: the
// ten sums of N (:241-250), ang (:266), nom / den (:282-294).
// cv::eigen is not available where this library is built.  The eigenvector of the largest eigenvalue of the symmetric 4x4 N comes
// from this project's own cyclic two-sided Jacobi in double on the float matrix (sim3_top_eigenvector on jacobi_internal.h), rounded to float as
// cv::eigen's float output is.  q and -q give the same rotation through the atan2 form of :266-273 (the axis flips and the angle
// 2 * ang becomes 2 * pi - 2 * ang), so the sign of the vector does not matter.  cv::Rodrigues works in double on the float vector and
// rounds the matrix to float; so does sim3_rodrigues.
// A quaternion with a zero imaginary part divides 0 by 0 at :268: everything behind it is NaN, every comparison of CheckInliers is
// false and the hypothesis has 0 inliers.  Nothing here branches on those values in a way that could trap or loop.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/orbfe.h"
#include "jacobi_internal.h"

#define SIM3_HD __host__ __device__ __forceinline__   // a call that is not inlined would pass the matrices through memory
#define SIM3_JACOBI_EPS 0x1p-53   // "diagonal to working precision"; a symmetric 4x4 converges in 4-7 sweeps

struct Sim3Prepared {   // one correspondence as iterate and CheckInliers read it: 48 bytes
  float c1[3], c2[3];   // mvX3Dc1[i], mvX3Dc2[i]
  float im1[2], im2[2]; // mvP1im1[i], mvP2im2[i]
  float max_err1, max_err2;
};

struct Sim3Transform {  // what ComputeSim3 leaves behind
  float s, R[9], t[3];  // ms12i, mR12i, mt12i
  float sR[9];          // the rotation block of mT12i
  float sRinv[9], tinv[3];   // mT21i
};

// R * x + t: the gemm's float dot in index order, then the addend (:93, :96, :367)
SIM3_HD void sim3_transform_point(const float* R, const float* t, const float* x, float* y) {
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = (R[3 * r] * x[0] + R[3 * r + 1] * x[1] + R[3 * r + 2] * x[2]) + t[r];
}

// FromCameraToImage / the tail of Project (:368-372, :387-391)
SIM3_HD void sim3_to_image(const orbfe_sim3_view& V, const float* c, float* im) {
  const float invz = 1 / c[2];
  const float x = c[0] * invz, y = c[1] * invz;
  im[0] = V.fx * x + V.cx;
  im[1] = V.fy * y + V.cy;
}

// the constructor's loop body for one kept match (:85-96, :106-107); the bounds arrive truncated
SIM3_HD void sim3_prepare(const orbfe_sim3_view& V1, const orbfe_sim3_view& V2, const orbfe_sim3_pair& p, Sim3Prepared& q) {
  sim3_transform_point(V1.Rcw, V1.tcw, p.Xw1, q.c1);
  sim3_transform_point(V2.Rcw, V2.tcw, p.Xw2, q.c2);
  sim3_to_image(V1, q.c1, q.im1);
  sim3_to_image(V2, q.c2, q.im2);
  q.max_err1 = p.max_err1;
  q.max_err2 = p.max_err2;
}

// One rotation of the two-sided Jacobi in the (p, q) plane of a symmetric 4x4: app, aqq, apq and the couplings of p and q with the
// two other indices (a_pk, a_qk, a_pl, a_ql), plus columns p and q of V.  Returns whether it rotated.
SIM3_HD bool sim3_rotate(double& app, double& aqq, double& apq, double& apk, double& aqk, double& apl, double& aql, double& v0p,
                         double& v1p, double& v2p, double& v3p, double& v0q, double& v1q, double& v2q, double& v3q) {
  if (jacobi_diagonal(app, aqq, apq, SIM3_JACOBI_EPS)) return false;
  double t, c, s;
  jacobi_rotation(app, aqq, apq, t, c, s);
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  double x;
  x = apk; apk = c * x - s * aqk; aqk = s * x + c * aqk;
  x = apl; apl = c * x - s * aql; aql = s * x + c * aql;
  x = v0p; v0p = c * x - s * v0q; v0q = s * x + c * v0q;
  x = v1p; v1p = c * x - s * v1q; v1q = s * x + c * v1q;
  x = v2p; v2p = c * x - s * v2q; v2q = s * x + c * v2q;
  x = v3p; v3p = c * x - s * v3q; v3q = s * x + c * v3q;
  return true;
}

// evec.row(0) of cv::eigen(N, eval, evec) (:259) up to sign, as floats: the unit eigenvector of the largest eigenvalue of the
// symmetric float 4x4 whose upper triangle is n00 .. n33.  N has trace 0 and is indefinite, hence the two-sided method (the
// one-sided Jacobi of mapping_internal.h yields singular vectors).  Every element is a named scalar: nothing lives in scratch.
SIM3_HD void sim3_top_eigenvector(float n00, float n01, float n02, float n03, float n11, float n12, float n13, float n22, float n23,
                                  float n33, float* q) {
  double a00 = n00, a01 = n01, a02 = n02, a03 = n03, a11 = n11, a12 = n12, a13 = n13, a22 = n22, a23 = n23, a33 = n33;
  double v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0;
  double v20 = 0, v21 = 0, v22 = 1, v23 = 0, v30 = 0, v31 = 0, v32 = 0, v33 = 1;
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
    bool rotated = false;
    rotated |= sim3_rotate(a00, a11, a01, a02, a12, a03, a13, v00, v10, v20, v30, v01, v11, v21, v31);   // (0, 1)
    rotated |= sim3_rotate(a00, a22, a02, a01, a12, a03, a23, v00, v10, v20, v30, v02, v12, v22, v32);   // (0, 2)
    rotated |= sim3_rotate(a00, a33, a03, a01, a13, a02, a23, v00, v10, v20, v30, v03, v13, v23, v33);   // (0, 3)
    rotated |= sim3_rotate(a11, a22, a12, a01, a02, a13, a23, v01, v11, v21, v31, v02, v12, v22, v32);   // (1, 2)
    rotated |= sim3_rotate(a11, a33, a13, a01, a03, a12, a23, v01, v11, v21, v31, v03, v13, v23, v33);   // (1, 3)
    rotated |= sim3_rotate(a22, a33, a23, a02, a03, a12, a13, v02, v12, v22, v32, v03, v13, v23, v33);   // (2, 3)
    if (!rotated) break;
  }
  // the first of equal eigenvalues; the column is taken by 0 / 1 weights, not by an index
  const double d[4] = {a00, a11, a22, a33};
  double s[4];
  jacobi_first_max(d, s);
  q[0] = (float)(v00 * s[0] + v01 * s[1] + v02 * s[2] + v03 * s[3]);
  q[1] = (float)(v10 * s[0] + v11 * s[1] + v12 * s[2] + v13 * s[3]);
  q[2] = (float)(v20 * s[0] + v21 * s[1] + v22 * s[2] + v23 * s[3]);
  q[3] = (float)(v30 * s[0] + v31 * s[1] + v32 * s[2] + v33 * s[3]);
}

// cv::Rodrigues of a float rotation vector into a float matrix: theta, the unit axis and the matrix in double, rounded once
SIM3_HD void sim3_rodrigues(const float* rv, float* R) {
  const double x = rv[0], y = rv[1], z = rv[2];
  const double theta = sqrt(x * x + y * y + z * z);
  if (theta < 2.220446049250313e-16) {   // DBL_EPSILON: the identity
    R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
    return;
  }
  const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
  const double ax = x * it, ay = y * it, az = z * it;
  R[0] = (float)(c + c1 * ax * ax);      R[1] = (float)(c1 * ax * ay - s * az); R[2] = (float)(c1 * ax * az + s * ay);
  R[3] = (float)(c1 * ax * ay + s * az); R[4] = (float)(c + c1 * ay * ay);      R[5] = (float)(c1 * ay * az - s * ax);
  R[6] = (float)(c1 * ax * az - s * ay); R[7] = (float)(c1 * ay * az + s * ax); R[8] = (float)(c + c1 * az * az);
}

// ComputeSim3 (:216-322): P1 = the three mvX3Dc1 of the triple (a, b, c), P2 the three mvX3Dc2
SIM3_HD void sim3_horn(const float* a1, const float* b1, const float* c1, const float* a2, const float* b2, const float* c2, bool fix_scale,
                       Sim3Transform& T) {
  // Step 1 (:207-214): cv::reduce sums in float, `C / P.cols` multiplies by (float)(1.0 / 3)
  const float third = (float)(1.0 / 3.0);
  float O1[3], O2[3], p1[9], p2[9];   // Pr1, Pr2: 3 x 3, column i = point i, row-major
#pragma unroll
  for (int r = 0; r < 3; r++) {
    O1[r] = ((a1[r] + b1[r]) + c1[r]) * third;
    O2[r] = ((a2[r] + b2[r]) + c2[r]) * third;
    p1[3 * r] = a1[r] - O1[r]; p1[3 * r + 1] = b1[r] - O1[r]; p1[3 * r + 2] = c1[r] - O1[r];
    p2[3 * r] = a2[r] - O2[r]; p2[3 * r + 1] = b2[r] - O2[r]; p2[3 * r + 2] = c2[r] - O2[r];
  }
  // Step 2 (:233): M = Pr2 * Pr1^T
  float M[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) M[3 * i + j] = p2[3 * i] * p1[3 * j] + p2[3 * i + 1] * p1[3 * j + 1] + p2[3 * i + 2] * p1[3 * j + 2];
  // Step 3 (:241-253): double sums of float entries, stored into a float matrix
  const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
  const float N11 = (float)(m00 + m11 + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10);
  const float N22 = (float)(m00 - m11 - m22), N23 = (float)(m01 + m10), N24 = (float)(m20 + m02);
  const float N33 = (float)(-m00 + m11 - m22), N34 = (float)(m12 + m21), N44 = (float)(-m00 - m11 + m22);
  // Step 4 (:257-273)
  float q[4];
  sim3_top_eigenvector(N11, N12, N13, N14, N22, N23, N24, N33, N34, N44, q);
  const double nv = sqrt((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2] + (double)q[3] * (double)q[3]);   // norm(vec)
  const double ang = atan2(nv, (double)q[0]);
  const float k = (float)(2 * ang / nv);   // 0 / 0 for a pure-real quaternion: NaN from here on, as in the reference
  const float rv[3] = {q[1] * k, q[2] * k, q[3] * k};
  sim3_rodrigues(rv, T.R);
  // Step 5 (:277): P3 = R * Pr2
  float P3[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) P3[3 * i + j] = T.R[3 * i] * p2[j] + T.R[3 * i + 1] * p2[3 + j] + T.R[3 * i + 2] * p2[6 + j];
  // Step 6 (:281-296)
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int e = 0; e < 9; e++) {
      nom += (double)p1[e] * (double)P3[e];
      den += (double)(P3[e] * P3[e]);   // cv::pow squares in float, the loop adds in double
    }
    T.s = (float)(nom / den);
  } else {
    T.s = 1.0f;
  }
  // Step 7 (:301): the gemm R * O2 with the scale folded in
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float ro = T.R[3 * r] * O2[0] + T.R[3 * r + 1] * O2[1] + T.R[3 * r + 2] * O2[2];
    T.t[r] = O1[r] - (float)((double)ro * (double)T.s);
  }
  // Step 8 (:306-321)
  const float inv_s = (float)(1.0 / (double)T.s);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      T.sR[3 * i + j] = T.s * T.R[3 * i + j];
      T.sRinv[3 * i + j] = inv_s * T.R[3 * j + i];
    }
#pragma unroll
  for (int r = 0; r < 3; r++) T.tinv[r] = -(T.sRinv[3 * r] * T.t[0] + T.sRinv[3 * r + 1] * T.t[1] + T.sRinv[3 * r + 2] * T.t[2]);
}

// CheckInliers for one correspondence (:326-338): err1 in image 1 of point 2 through T12, err2 in image 2 of point 1 through T21
SIM3_HD bool sim3_is_inlier(const orbfe_sim3_view& V1, const orbfe_sim3_view& V2, const float* sR, const float* t, const float* sRinv,
                            const float* tinv, const Sim3Prepared& p) {
  float c[3], im[2];
  sim3_transform_point(sR, t, p.c2, c);
  sim3_to_image(V1, c, im);
  const float d1x = p.im1[0] - im[0], d1y = p.im1[1] - im[1];
  sim3_transform_point(sRinv, tinv, p.c1, c);
  sim3_to_image(V2, c, im);
  const float d2x = im[0] - p.im2[0], d2y = im[1] - p.im2[1];
  const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);   // Mat::dot returns double
  const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
  return err1 < p.max_err1 && err2 < p.max_err2;
}

// true when (i0, i1, i2) can be a draw of :162-172: inside [0, n) and pairwise different
SIM3_HD bool sim3_triple_ok(int i0, int i1, int i2, int n) {
  return i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n && i0 != i1 && i0 != i2 && i1 != i2;
}

// ---- launchers (sim3_kernels.hip)
#define SIM3_WAVES 4   // hypotheses (waves) per workgroup
struct Sim3Launch {
  const orbfe_sim3_view* view1; const orbfe_sim3_view* view2;   // [P]
  const orbfe_sim3_pair* pairs; const int32_t* n; int cap;      // [P][cap], [P]
  const int32_t* triples; const int32_t* H; int h_cap;          // [P][h_cap][3], [P]
  const int32_t* fix_scale; const int32_t* min_inliers;         // [P]
  orbfe_sim3_hypothesis* hyps;                                  // [P][h_cap]
  uint64_t* words;                                              // [P][h_cap][W], W = ceil(cap / 64)
  orbfe_sim3_result* result; uint64_t* mask;                    // [P], [P][W]
};
void orbfe_launch_sim3_hypotheses(const Sim3Launch& L, int P, hipStream_t s);
void orbfe_launch_sim3_select(const Sim3Launch& L, int P, hipStream_t s);
