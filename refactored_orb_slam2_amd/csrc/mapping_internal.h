// mapping_internal.h -- the arithmetic of the triangulation half of LocalMapping::CreateNewMapPoints, once, for the kernel
// (mapping_kernels.hip) and for host code that wants the same bits.  __host__ __device__ inline functions, compiled with
// -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   LocalMapping::CreateNewMapPoints, per match   L/src/LocalMapping.cc:261-402
//   the baseline gate per neighbour               L/src/LocalMapping.cc:221-235
//   KeyFrame::UnprojectStereo                     L/src/KeyFrame.cc:573-586
//   MapPoint::UpdateNormalAndDepth                L/src/MapPoint.cc:340-381
// cv::Mat arithmetic is read as frustum_kernels.hip reads it (OpenCV 4.5's small-matrix paths): a matrix product is a float dot
// product per element in index order (the double epilogue `* alpha` is the identity without an addend and `+ beta * C` is one
// double addition), Mat::dot and cv::norm accumulate in double in element order, `Mat / scalar` multiplies by (float)(1.0 / scalar).
// `cos` and `atan2` at :289-292 are the FLOAT overloads: the file says `using namespace ::std` and every argument is a float
// (mb / 2, mvDepth[i], 2 * float), so overload resolution picks std::atan2(float, float) and std::cos(float).  The device has no
// glibc: both are evaluated in double and rounded to float, which is the correctly rounded float result except for double-rounding
// cases, i.e. within an ulp of any faithful float libm.
// cv::SVD is not available where this library is built; the null vector of the 4x4 comes from this project's own one-sided
// Jacobi in double on the float matrix (tri_null_vector on jacobi_internal.h), rounded to float.  x3D does not depend on the sign of the vector.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/orbfe.h"
#include "jacobi_internal.h"

#define TRI_HD __host__ __device__ __forceinline__   // a call that is not inlined would pass the 4x4 through memory
#define TRI_JACOBI_EPS 0x1p-50   // "orthogonal to working precision" of the float 4x4; a 4x4 converges in 4-6 sweeps

// ---- cv::Mat helpers (the evaluation order of frustum_kernels.hip)
// (R^T * x)[r]: Rwc = Rcw.t(), then the gemm's float dot in index order (:196, :279)
TRI_HD float tri_rt_row(const float* R, int r, float x, float y, float z) { return R[r] * x + R[3 + r] * y + R[6 + r] * z; }
// R.row(r).dot(x3Dt) + t: Mat::dot returns double, the float addend widens, the sum is rounded once (:327)
TRI_HD float tri_row_dot(const float* R, int r, const float* x, float t) {
  double s = 0.0;
  s += (double)R[3 * r] * (double)x[0];
  s += (double)R[3 * r + 1] * (double)x[1];
  s += (double)R[3 * r + 2] * (double)x[2];
  return (float)(s + (double)t);
}
TRI_HD double tri_dot3(const float* a, const float* b) {
  double s = 0.0;
  s += (double)a[0] * (double)b[0];
  s += (double)a[1] * (double)b[1];
  s += (double)a[2] * (double)b[2];
  return s;
}
TRI_HD double tri_norm3(const float* a) { return sqrt(tri_dot3(a, a)); }

// cos(2 * atan2(mb / 2, depth)) with the float overloads (:289-292)
TRI_HD float tri_cos_parallax_stereo(float mb, float depth) {
  const float a = (float)atan2((double)(mb / 2), (double)depth);
  return (float)cos((double)(2 * a));
}

// One rotation of the one-sided Jacobi: columns p and q of A (4 rows) and of V are rotated so that the two columns of A become
// orthogonal.  Returns whether it rotated.
TRI_HD bool tri_rotate(double& a0p, double& a1p, double& a2p, double& a3p, double& a0q, double& a1q, double& a2q,
                                           double& a3q, double& v0p, double& v1p, double& v2p, double& v3p, double& v0q, double& v1q,
                                           double& v2q, double& v3q) {
  const double alpha = a0p * a0p + a1p * a1p + a2p * a2p + a3p * a3p;
  const double beta = a0q * a0q + a1q * a1q + a2q * a2q + a3q * a3q;
  const double gamma = a0p * a0q + a1p * a1q + a2p * a2q + a3p * a3q;
  double c, s;
  if (!jacobi_onesided_rotation(alpha, beta, gamma, TRI_JACOBI_EPS, c, s)) return false;
  double x;
  x = a0p; a0p = c * x - s * a0q; a0q = s * x + c * a0q;
  x = a1p; a1p = c * x - s * a1q; a1q = s * x + c * a1q;
  x = a2p; a2p = c * x - s * a2q; a2q = s * x + c * a2q;
  x = a3p; a3p = c * x - s * a3q; a3q = s * x + c * a3q;
  x = v0p; v0p = c * x - s * v0q; v0q = s * x + c * v0q;
  x = v1p; v1p = c * x - s * v1q; v1q = s * x + c * v1q;
  x = v2p; v2p = c * x - s * v2q; v2q = s * x + c * v2q;
  x = v3p; v3p = c * x - s * v3q; v3q = s * x + c * v3q;
  return true;
}

// The right singular vector of the smallest singular value of the float 4x4 A (row-major), as floats: vt.row(3) of :307-309 up
// to sign.  One-sided (Hestenes) Jacobi in double: A V = U S, the singular values are the column norms of A V.  Every element is a
// named scalar, so a kernel keeps all of it in registers.
TRI_HD void tri_null_vector(const float* A, float* v) {
  double a00 = A[0], a01 = A[1], a02 = A[2], a03 = A[3], a10 = A[4], a11 = A[5], a12 = A[6], a13 = A[7];
  double a20 = A[8], a21 = A[9], a22 = A[10], a23 = A[11], a30 = A[12], a31 = A[13], a32 = A[14], a33 = A[15];
  double v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0;
  double v20 = 0, v21 = 0, v22 = 1, v23 = 0, v30 = 0, v31 = 0, v32 = 0, v33 = 1;
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
    bool rotated = false;
    rotated |= tri_rotate(a00, a10, a20, a30, a01, a11, a21, a31, v00, v10, v20, v30, v01, v11, v21, v31);   // (0, 1)
    rotated |= tri_rotate(a00, a10, a20, a30, a02, a12, a22, a32, v00, v10, v20, v30, v02, v12, v22, v32);   // (0, 2)
    rotated |= tri_rotate(a00, a10, a20, a30, a03, a13, a23, a33, v00, v10, v20, v30, v03, v13, v23, v33);   // (0, 3)
    rotated |= tri_rotate(a01, a11, a21, a31, a02, a12, a22, a32, v01, v11, v21, v31, v02, v12, v22, v32);   // (1, 2)
    rotated |= tri_rotate(a01, a11, a21, a31, a03, a13, a23, a33, v01, v11, v21, v31, v03, v13, v23, v33);   // (1, 3)
    rotated |= tri_rotate(a02, a12, a22, a32, a03, a13, a23, a33, v02, v12, v22, v32, v03, v13, v23, v33);   // (2, 3)
    if (!rotated) break;
  }
  const double n0 = a00 * a00 + a10 * a10 + a20 * a20 + a30 * a30, n1 = a01 * a01 + a11 * a11 + a21 * a21 + a31 * a31;
  const double n2 = a02 * a02 + a12 * a12 + a22 * a22 + a32 * a32, n3 = a03 * a03 + a13 * a13 + a23 * a23 + a33 * a33;
  // the first of equal norms, its column taken by 0 / 1 weights: jacobi_first_min written out (the call moves instructions of the
  // kernel's tail, and this listing is held to the last line)
  int j = 0;
  double m = n0;
  if (n1 < m) { m = n1; j = 1; }
  if (n2 < m) { m = n2; j = 2; }
  if (n3 < m) { m = n3; j = 3; }
  const double s0 = j == 0 ? 1.0 : 0.0, s1 = j == 1 ? 1.0 : 0.0, s2 = j == 2 ? 1.0 : 0.0, s3 = j == 3 ? 1.0 : 0.0;
  const double w0 = v00 * s0 + v01 * s1 + v02 * s2 + v03 * s3, w1 = v10 * s0 + v11 * s1 + v12 * s2 + v13 * s3;
  const double w2 = v20 * s0 + v21 * s1 + v22 * s2 + v23 * s3, w3 = v30 * s0 + v31 * s1 + v32 * s2 + v33 * s3;
  v[0] = (float)w0; v[1] = (float)w1; v[2] = (float)w2; v[3] = (float)w3;
}

struct TriObs {   // one keypoint as the loop body reads it
  float x, y, u_right, depth;   // mvKeysUn[i].pt, mvuRight[i] (< 0: monocular), mvDepth[i]
  int octave;                   // in [0, n_levels) of its view: the caller has checked
};

// `errX * errX + errY * errY (+ errXr * errXr) > 5.991 | 7.8 * sigma2` of :341-358 and :365-382; mbf is pKF1's in both (:350, :374)
TRI_HD bool tri_reproj_fails(const orbfe_tri_view& V, const TriObs& o, bool stereo, const float* x3D, float z, float mbf,
                                                 float sigma2) {
  const float x = tri_row_dot(V.Rcw, 0, x3D, V.tcw[0]);
  const float y = tri_row_dot(V.Rcw, 1, x3D, V.tcw[1]);
  const float invz = (float)(1.0 / (double)z);
  const float u = V.fx * x * invz + V.cx;
  if (!stereo) {
    const float v = V.fy * y * invz + V.cy;
    const float ex = u - o.x, ey = v - o.y;
    return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
  }
  const float u_r = u - mbf * invz;
  const float v = V.fy * y * invz + V.cy;
  const float ex = u - o.x, ey = v - o.y, er = u_r - o.u_right;
  return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// KeyFrame::UnprojectStereo (KeyFrame.cc:573-586) from the undistorted keypoint (the reference reads mvKeys: equal for the
// rectified stereo and undistorted RGB-D input this library produces); Twc's rotation is Rcw.t(), its translation Ow
TRI_HD void tri_unproject(const orbfe_tri_view& V, const TriObs& o, float* x3D) {
  const float z = o.depth;
  const float x = (o.x - V.cx) * z * V.invfx;
  const float y = (o.y - V.cy) * z * V.invfy;
#pragma unroll
  for (int r = 0; r < 3; r++) x3D[r] = (float)((double)tri_rt_row(V.Rcw, r, x, y, z) * 1.0 + (double)V.Ow[r] * 1.0);
}

// The body of the match loop (:261-421) up to `new MapPoint`, plus what UpdateNormalAndDepth (:415) computes for the new point.
// s1 / s2: mvLevelSigma2 and mvScaleFactors of the two keypoints' octaves; s1_top: pKF1's mvScaleFactors[nLevels - 1].
// Writes pos / normal / min_distance / max_distance of P for an accepted pair; returns the code and *path.
TRI_HD int tri_pair(const orbfe_tri_view& V1, const orbfe_tri_view& V2, const TriObs& o1, const TriObs& o2, float sigma2_1,
                                        float sigma2_2, float sf1, float sf2, float sf1_top, float ratio_factor, orbfe_new_point& P,
                                        int* path) {
  const bool bStereo1 = o1.u_right >= 0, bStereo2 = o2.u_right >= 0;
  *path = ORBFE_TRI_PATH_NONE;
  // :274-282
  const float xn1[3] = {(o1.x - V1.cx) * V1.invfx, (o1.y - V1.cy) * V1.invfy, 1.0f};
  const float xn2[3] = {(o2.x - V2.cx) * V2.invfx, (o2.y - V2.cy) * V2.invfy, 1.0f};
  float ray1[3], ray2[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    ray1[r] = tri_rt_row(V1.Rcw, r, xn1[0], xn1[1], xn1[2]);
    ray2[r] = tri_rt_row(V2.Rcw, r, xn2[0], xn2[1], xn2[2]);
  }
  const float cosParallaxRays = (float)(tri_dot3(ray1, ray2) / (tri_norm3(ray1) * tri_norm3(ray2)));
  // :284-294
  float cosParallaxStereo = cosParallaxRays + 1;
  float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
  if (bStereo1) cosParallaxStereo1 = tri_cos_parallax_stereo(V1.mb, o1.depth);
  else if (bStereo2) cosParallaxStereo2 = tri_cos_parallax_stereo(V2.mb, o2.depth);
  cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min(a, b): b < a ? b : a
  float x3D[3];
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
    // :300-315; `s * row - row` is the float product, then the float difference
    float A[16], v[4];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      A[j] = xn1[0] * V1.Rcw[6 + j] - V1.Rcw[j];
      A[4 + j] = xn1[1] * V1.Rcw[6 + j] - V1.Rcw[3 + j];
      A[8 + j] = xn2[0] * V2.Rcw[6 + j] - V2.Rcw[j];
      A[12 + j] = xn2[1] * V2.Rcw[6 + j] - V2.Rcw[3 + j];
    }
    A[3] = xn1[0] * V1.tcw[2] - V1.tcw[0];
    A[7] = xn1[1] * V1.tcw[2] - V1.tcw[1];
    A[11] = xn2[0] * V2.tcw[2] - V2.tcw[0];
    A[15] = xn2[1] * V2.tcw[2] - V2.tcw[1];
    tri_null_vector(A, v);
    *path = ORBFE_TRI_PATH_LINEAR;
    if (v[3] == 0) return ORBFE_TRI_W_ZERO;
    const float inv_w = (float)(1.0 / (double)v[3]);
    x3D[0] = v[0] * inv_w; x3D[1] = v[1] * inv_w; x3D[2] = v[2] * inv_w;
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2 && o1.depth > 0) {
    tri_unproject(V1, o1, x3D);
    *path = ORBFE_TRI_PATH_UNPROJECT1;
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1 && o2.depth > 0) {
    tri_unproject(V2, o2, x3D);
    *path = ORBFE_TRI_PATH_UNPROJECT2;
  } else {
    return ORBFE_TRI_LOW_PARALLAX;   // :322 (and a stereo keypoint without a positive depth, which the reference never has)
  }
  // :327-333
  const float z1 = tri_row_dot(V1.Rcw, 2, x3D, V1.tcw[2]);
  if (z1 <= 0) return ORBFE_TRI_BEHIND1;
  const float z2 = tri_row_dot(V2.Rcw, 2, x3D, V2.tcw[2]);
  if (z2 <= 0) return ORBFE_TRI_BEHIND2;
  // :336-382
  if (tri_reproj_fails(V1, o1, bStereo1, x3D, z1, V1.mbf, sigma2_1)) return ORBFE_TRI_REPROJ1;
  if (tri_reproj_fails(V2, o2, bStereo2, x3D, z2, V1.mbf, sigma2_2)) return ORBFE_TRI_REPROJ2;
  // :385-402
  const float normal1[3] = {x3D[0] - V1.Ow[0], x3D[1] - V1.Ow[1], x3D[2] - V1.Ow[2]};
  const float normal2[3] = {x3D[0] - V2.Ow[0], x3D[1] - V2.Ow[1], x3D[2] - V2.Ow[2]};
  const double n1 = tri_norm3(normal1), n2 = tri_norm3(normal2);
  const float dist1 = (float)n1, dist2 = (float)n2;
  if (dist1 == 0 || dist2 == 0) return ORBFE_TRI_DIST_ZERO;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = sf1 / sf2;
  if (ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor) return ORBFE_TRI_SCALE;
  // MapPoint::UpdateNormalAndDepth (MapPoint.cc:357-380) with the observations {pKF1, pKF2} and pRefKF = pKF1: the sum of the
  // two unit vectors does not depend on the order the std::map yields them in (0 + a is exact, a + b commutes)
  const float r1 = (float)(1.0 / n1), r2 = (float)(1.0 / n2);   // normali / cv::norm(normali)
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float sum = (0.0f + normal1[k] * r1) + normal2[k] * r2;
    P.pos[k] = x3D[k];
    P.normal[k] = sum * 0.5f;   // normal / n, n = 2
  }
  P.max_distance = dist1 * sf1;                  // :377
  P.min_distance = P.max_distance / sf1_top;     // :378
  return ORBFE_TRI_OK;
}

// The baseline gate of :221-235: true = the neighbour is skipped
TRI_HD bool tri_baseline_too_short(const float* Ow1, const float* Ow2, int monocular, float mb2, float median_depth2) {
  const float d[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
  const float baseline = (float)tri_norm3(d);
  if (!monocular) return baseline < mb2;
  const float ratioBaselineDepth = baseline / median_depth2;
  return (double)ratioBaselineDepth < 0.01;
}

// ---- launchers (mapping_kernels.hip)
struct TriLaunch {
  const orbfe_tri_view* view1;     // ONE record
  const orbfe_keypoint* keys1; const float* u_right1; const float* depth1;   // [capA] (u_right / depth nullable: all monocular)
  const int32_t* nA; int nA_host;  // rows of pair k: nA[k] when nA != NULL, else nA_host for every k; clamped to [0, capA]
  int capA;
  const orbfe_tri_view* view2;     // [K]
  const orbfe_keypoint* keys2; const float* u_right2; const float* depth2;   // [K][capB]
  const int32_t* nB; int nB_host; int capB;
  const int32_t* matchA;           // [K][capA]
  orbfe_new_point* out;            // [K][capA]
  uint8_t* validA;                 // chained form: candidate mask of the next search, cleared at accepted rows; else NULL
};
void orbfe_launch_triangulate(const TriLaunch& t, int K, hipStream_t s);
// n_new[k] = accepted rows of pair k; n_matches[k] = counters[k * counter_stride + 1] when counters != NULL
void orbfe_launch_triangulate_count(const orbfe_new_point* out, const int32_t* nA, int nA_host, int capA, int32_t* n_new,
                                    const int32_t* counters, int counter_stride, int32_t* n_matches, int K, hipStream_t s);
