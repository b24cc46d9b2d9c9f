// optsim3_internal.h -- the arithmetic of Optimizer::OptimizeSim3, once, for the kernel (optsim3_kernels.hip) and for host code that
// wants the same bits.  __host__ __device__ inline functions, all in double, compiled with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/, G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o/):
//   Optimizer::OptimizeSim3                       L/src/Optimizer.cc:1381-1573
//   Sim3(Matrix3, Vector3, double), Sim3(Vector7) G/types/sim3/sim3.h:56-59, :61-124
//   Sim3::map, inverse, operator*, normalize      G/types/sim3/sim3.h:126, :200-202, :226-232, :239-244
//   VertexSim3Expmap::oplusImpl, cam_map1 / 2     G/types/sim3/types_seven_dof_expmap.h:77-84, :113-125
//   EdgeSim3ProjectXYZ / EdgeInverseSim3...       G/types/sim3/types_seven_dof_expmap.h:180-187, :201-209 (no linearizeOplus: :189, :211)
//   project                                       G/types/slam3d/se3_ops.hpp:47-52
//   numeric Jacobian (linearizeOplusN)            G/core/base_fixed_sized_edge.hpp:152-209
// Sim3 holds its rotation and translation as pose_internal.h's SE3Quat does, with that header's quaternion formulas; the optimiser
// around the edges is lm_internal.h's, for a vertex of 7 dimensions; the camera-frame points are sim3_internal.h's float gemm
// (Optimizer.cc:1452, :1460).  BlockSolverX with LinearSolverEigen factorises the one 7 x 7 block with SimplicialLLT; here it is
// lm_internal.h's unpivoted L D L^T, as for the pose reading's dense solver.  A reading, unpinned.
//
// The edges have no analytic Jacobian: column d of both is the central difference (e(+delta e_d) - e(-delta e_d)) / (2 delta) with
// delta = 1e-9 through oplus, i.e. through Sim3(update) * estimate.  With a fixed scale oplus zeroes update[6] before it is used, so
// both perturbed estimates of column 6 are the same and the column is exactly zero: H[6][6] is lambda alone and x[6] == 0.
// Sim3(Vector7) does not normalise its quaternion and operator* does not either; inverse() does (through the constructor).
#pragma once
#include "lm_internal.h"
#include "pose_internal.h"
#include "sim3_internal.h"

constexpr int OS_NACC = lm_nacc<7>;   // 28 upper entries of H, 7 of b, chi
#define OS_NTRANSFORMS 15   // the estimate, then (+delta, -delta) of each of the 7 dimensions

struct OsSim3 {   // g2o::Sim3: rotation and translation as PoseSE3 holds them, and the scale
  PoseSE3 q;
  double s;
};

struct OsCam {   // _focal_length, _principle_point of one keyframe: mK's floats widened (Optimizer.cc:1411-1418)
  double fx, fy, cx, cy;
};

struct OsPair {   // one correspondence as the two edges read it: every value a float widened
  double x1, y1, z1;   // P3D1c
  double x2, y2, z2;   // P3D2c
  double u1, v1, u2, v2;
  double w1, w2;       // information = w * I
};

// `const float deltaHuber = sqrt(th2)` (Optimizer.cc:1432)
__host__ __device__ inline double os_delta(float th2) { return (double)sqrtf(th2); }

// Sim3(Matrix3, Vector3, double) of the floats s, R[9], t[3] (LoopClosing.cc builds g2oS12 from float matrices)
__host__ __device__ inline OsSim3 os_from_floats(const float* v) {
  OsSim3 S;
  pose_quat_from_matrix((double)v[1], (double)v[2], (double)v[3], (double)v[4], (double)v[5], (double)v[6], (double)v[7], (double)v[8],
                        (double)v[9], S.q);
  S.q.tx = (double)v[10];
  S.q.ty = (double)v[11];
  S.q.tz = (double)v[12];
  S.s = (double)v[0];
  pose_normalize(S.q);
  return S;
}

// scale(), rotation().toRotationMatrix(), translation() rounded to float
__host__ __device__ inline void os_to_floats(const OsSim3& S, float* v) {
  float T[12];
  pose_to_Tcw(S.q, T);
  v[0] = (float)S.s;
  v[1] = T[0]; v[2] = T[1]; v[3] = T[2];
  v[4] = T[4]; v[5] = T[5]; v[6] = T[6];
  v[7] = T[8]; v[8] = T[9]; v[9] = T[10];
  v[10] = T[3]; v[11] = T[7]; v[12] = T[11];
}

// Sim3(const Vector7&): omega, upsilon, sigma
__host__ __device__ inline OsSim3 os_exp(const double* u) {
  const double sigma = u[6];
  const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double Om[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
  OsSim3 S;
  S.s = exp(sigma);
  double Om2[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Om2[i][j] = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j];
  const double eps = 0.00001;
  double A, B, Cc, ra, rb;   // R = I + ra * Omega + rb * Omega2 (small angle: I + Omega + Omega2 / 2)
  const bool small_angle = theta < eps;
  if (small_angle) {
    ra = 1.0;
    rb = 0.5;
  } else {
    ra = sin(theta) / theta;
    rb = (1 - cos(theta)) / (theta * theta);
  }
  if (fabs(sigma) < eps) {
    Cc = 1;
    if (small_angle) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    Cc = (S.s - 1) / sigma;
    if (small_angle) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * S.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * S.s - 1) / (sigma2 * sigma);
    } else {
      const double a = S.s * sin(theta);
      const double b = S.s * cos(theta);
      const double theta2 = theta * theta;
      const double sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (Cc - ((b - 1) * sigma + a * theta) / (c)) * 1 / (theta2);
    }
  }
  double R[3][3], W[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double eye = i == j ? 1.0 : 0.0;
      R[i][j] = small_angle ? eye + Om[i][j] + Om2[i][j] / 2 : eye + ra * Om[i][j] + rb * Om2[i][j];
      W[i][j] = A * Om[i][j] + B * Om2[i][j] + Cc * eye;
    }
  pose_quat_from_matrix(R[0][0], R[0][1], R[0][2], R[1][0], R[1][1], R[1][2], R[2][0], R[2][1], R[2][2], S.q);
  S.q.tx = W[0][0] * u[3] + W[0][1] * u[4] + W[0][2] * u[5];
  S.q.ty = W[1][0] * u[3] + W[1][1] * u[4] + W[1][2] * u[5];
  S.q.tz = W[2][0] * u[3] + W[2][1] * u[4] + W[2][2] * u[5];
  return S;
}

// Sim3::map: s * (r * xyz) + t
__host__ __device__ inline void os_map(const OsSim3& S, double X, double Y, double Z, double* x, double* y, double* z) {
  double rx, ry, rz;
  pose_rotate(S.q, X, Y, Z, &rx, &ry, &rz);
  *x = S.s * rx + S.q.tx;
  *y = S.s * ry + S.q.ty;
  *z = S.s * rz + S.q.tz;
}

// Sim3::operator*: Eigen's quaternion product, no normalisation
__host__ __device__ inline OsSim3 os_mul(const OsSim3& a, const OsSim3& b) {
  OsSim3 r;
  os_map(a, b.q.tx, b.q.ty, b.q.tz, &r.q.tx, &r.q.ty, &r.q.tz);
  r.q.qx = a.q.qw * b.q.qx + a.q.qx * b.q.qw + a.q.qy * b.q.qz - a.q.qz * b.q.qy;
  r.q.qy = a.q.qw * b.q.qy + a.q.qy * b.q.qw + a.q.qz * b.q.qx - a.q.qx * b.q.qz;
  r.q.qz = a.q.qw * b.q.qz + a.q.qz * b.q.qw + a.q.qx * b.q.qy - a.q.qy * b.q.qx;
  r.q.qw = a.q.qw * b.q.qw - a.q.qx * b.q.qx - a.q.qy * b.q.qy - a.q.qz * b.q.qz;
  r.s = a.s * b.s;
  return r;
}

// Sim3::inverse: Sim3(r.conjugate(), r.conjugate() * ((-1 / s) * t), 1 / s), whose constructor normalises
__host__ __device__ inline OsSim3 os_inverse(const OsSim3& S) {
  OsSim3 r;
  r.q.qx = -S.q.qx;
  r.q.qy = -S.q.qy;
  r.q.qz = -S.q.qz;
  r.q.qw = S.q.qw;
  const double k = -1 / S.s;
  pose_rotate(r.q, k * S.q.tx, k * S.q.ty, k * S.q.tz, &r.q.tx, &r.q.ty, &r.q.tz);
  r.s = 1 / S.s;
  pose_normalize(r.q);
  return r;
}

// VertexSim3Expmap::oplusImpl
__host__ __device__ inline OsSim3 os_oplus(const OsSim3& S, const double* update, bool fix_scale) {
  const double u[7] = {update[0], update[1], update[2], update[3], update[4], update[5], fix_scale ? 0.0 : update[6]};
  return os_mul(os_exp(u), S);
}

// The estimate perturbed for the numeric Jacobian: j = 0 the estimate itself, j = 1 + 2 d the step +delta along dimension d,
// j = 2 + 2 d the step -delta.  The update vector is written by comparisons, not through an index.
__host__ __device__ inline OsSim3 os_perturbed(const OsSim3& S, int j, bool fix_scale) {
  if (j == 0) return S;
  const int d = (j - 1) >> 1;
  const double step = ((j - 1) & 1) ? -1e-9 : 1e-9;
  const double u[7] = {d == 0 ? step : 0.0, d == 1 ? step : 0.0, d == 2 ? step : 0.0, d == 3 ? step : 0.0,
                       d == 4 ? step : 0.0, d == 5 ? step : 0.0, d == 6 ? step : 0.0};
  return os_oplus(S, u, fix_scale);
}

// obs - cam_map(project(T.map(P))): the error of EdgeSim3ProjectXYZ with (T, P, K, obs) = (S12, P2c, K1, obs1), of
// EdgeInverseSim3ProjectXYZ with (S12.inverse(), P1c, K2, obs2)
__host__ __device__ inline void os_error(const OsSim3& T, const OsCam& K, double X, double Y, double Z, double ou, double ov, double* e0,
                                         double* e1) {
  double x, y, z;
  os_map(T, X, Y, Z, &x, &y, &z);
  *e0 = ou - (x / z * K.fx + K.cx);
  *e1 = ov - (y / z * K.fy + K.cy);
}

// chi2() = error . (information * error)
__host__ __device__ inline double os_chi2(double e0, double e1, double w) { return e0 * (w * e0) + e1 * (w * e1); }

// scalar * (e(+) - e(-)) of linearizeOplusN, scalar = 1 / (2 * delta)
__host__ __device__ inline double os_central(double ep, double em) { return (1 / (2 * 1e-9)) * (ep - em); }

// one correspondence from the caller's record: the camera-frame points in float, everything widened
__host__ __device__ inline void os_prepare(const orbfe_sim3_view& V1, const orbfe_sim3_view& V2, const orbfe_optsim3_pair& p, float* c1,
                                           float* c2) {
  sim3_transform_point(V1.Rcw, V1.tcw, p.Xw1, c1);
  sim3_transform_point(V2.Rcw, V2.tcw, p.Xw2, c2);
}

#define OS_MAX_PROBLEMS 65535
struct OsLaunch {
  const orbfe_sim3_view* view1; const orbfe_sim3_view* view2;   // [P]
  const orbfe_optsim3_pair* pairs; const int32_t* n; int cap;   // [P][cap], [P]
  const float* s_R_t_in;                                        // [P][13]
  const float* th2; const int32_t* fix_scale;                   // [P]
  orbfe_optsim3_result* result; uint8_t* bad;                   // [P], [P][cap]
};
void orbfe_launch_optimize_sim3(const OsLaunch& L, int P, hipStream_t s);
