// egraph_internal.h -- the arithmetic of Optimizer::OptimizeEssentialGraph and of the map correction behind it, once, for the kernels
// (egraph_kernels.hip) and for host code that wants the same bits.  __host__ __device__ inline functions, all in double, compiled
// with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/, G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o/):
//   Optimizer::OptimizeEssentialGraph             L/src/Optimizer.cc:1366; the Sim3 form :760-1043, the SE3 form :1052-1362
//   Sim3::log                                     G/types/sim3/sim3.h:128-197 (W.lu().solve(t): Eigen's PartialPivLU of a 3 x 3)
//   EdgeSim3::computeError                        G/types/sim3/types_seven_dof_expmap.h:142-151 (no linearizeOplus: :166-168)
//   numeric Jacobian (linearizeOplusN)            G/core/base_fixed_sized_edge.hpp:152-209
//   SE3Quat::log, inverse, adj                    G/types/slam3d/se3quat.h:165-198, :114-119, :232-240
//   EdgeSE3Expmap::computeError, linearizeOplus   G/types/sba/edge_se3_expmap.cpp:46-71
//   deltaR                                        G/types/slam3d/se3_ops.hpp:39-45
// Sim3's constructor, map, operator*, inverse and oplus are optsim3_internal.h's, SE3Quat's operator* and exp pose_internal.h's, the
// Levenberg rules lm_internal.h's.  A transform of either path is held in an OsSim3 (the SE3 path keeps s = 1 and never reads it).
// Neither Eigen nor g2o can be built where this library is built: fixed-size products are taken in index order, B * Omega * Omega is
// B * (Omega * Omega) as in os_exp.  A reading, unpinned.
#pragma once
#include "optsim3_internal.h"

constexpr double EG_SCALE_TOL = 1e-3;        // kScaleTol (Optimizer.cc:1057)
constexpr double EG_LAMBDA_INIT = 1e-16;     // setUserLambdaInit (:778, :1080): computeLambdaInit returns it as it is
constexpr int EG_ITERATIONS = 20;            // optimize(20)
constexpr int EG_EDGE_DOUBLES = 2 * 49 + 7;  // per edge in the workspace: the Jacobians of vertex 0 and 1 (column-major D x D), the error
constexpr int EG_MAX_POINTS = 16777216;      // orbfe_sim3_correct_points

__host__ __device__ inline OsSim3 eg_load(const orbfe_eg_sim3& r) {
  OsSim3 S;
  S.q.qx = r.q[0]; S.q.qy = r.q[1]; S.q.qz = r.q[2]; S.q.qw = r.q[3];
  S.q.tx = r.t[0]; S.q.ty = r.t[1]; S.q.tz = r.t[2];
  S.s = r.s;
  return S;
}

__host__ __device__ inline void eg_store(const OsSim3& S, orbfe_eg_sim3& r) {
  r.q[0] = S.q.qx; r.q[1] = S.q.qy; r.q[2] = S.q.qz; r.q[3] = S.q.qw;
  r.t[0] = S.q.tx; r.t[1] = S.q.ty; r.t[2] = S.q.tz;
  r.s = S.s;
}

// the limits on a record: finite, s > 0, a quaternion of non-zero norm
__host__ __device__ inline bool eg_record_ok(const orbfe_eg_sim3& r) {
  const bool fin = isfinite(r.q[0]) && isfinite(r.q[1]) && isfinite(r.q[2]) && isfinite(r.q[3]) && isfinite(r.t[0]) && isfinite(r.t[1]) &&
                   isfinite(r.t[2]) && isfinite(r.s);
  const double n2 = r.q[0] * r.q[0] + r.q[1] * r.q[1] + r.q[2] * r.q[2] + r.q[3] * r.q[3];
  return fin && r.s > 0.0 && n2 > 0.0 && isfinite(n2);
}

// checkUnitScale (Optimizer.cc:1058-1067)
__host__ __device__ inline bool eg_unit_scale(double s) { return !(fabs(s - 1.0) > EG_SCALE_TOL); }

// the scale of the measurement Sj * Si^-1 as os_mul and os_inverse compute it: what the host checks without the rest
__host__ __device__ inline double eg_measurement_scale(double si, double sj) { return sj * (1 / si); }

// `Sjw * Swi` with Swi = Siw.inverse() (Optimizer.cc:846-858, :881-907)
__host__ __device__ inline OsSim3 eg_measurement(const OsSim3& Siw, const OsSim3& Sjw) { return os_mul(Sjw, os_inverse(Siw)); }

// SE3Quat(S.rotation(), S.translation()): the constructor normalises
__host__ __device__ inline OsSim3 eg_to_se3(const OsSim3& S) {
  OsSim3 T = S;
  pose_normalize(T.q);
  T.s = 1.0;
  return T;
}

// W.lu().solve(t): PartialPivLU of a 3 x 3 (the first largest |entry| of the column is the pivot), the unit lower solve, the upper
// solve.  Rows are exchanged by comparisons, never through an index.
__host__ __device__ inline void eg_lu_solve3(const double* W, const double* t, double* x) {
  double m[3][4] = {{W[0], W[1], W[2], t[0]}, {W[3], W[4], W[5], t[1]}, {W[6], W[7], W[8], t[2]}};
  {
    int p = 0;
    double big = fabs(m[0][0]);
    if (fabs(m[1][0]) > big) {
      p = 1;
      big = fabs(m[1][0]);
    }
    if (fabs(m[2][0]) > big) p = 2;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const double a = m[0][c], b1 = m[1][c], b2 = m[2][c];
      m[0][c] = p == 1 ? b1 : (p == 2 ? b2 : a);
      m[1][c] = p == 1 ? a : b1;
      m[2][c] = p == 2 ? a : b2;
    }
  }
  m[1][0] = m[1][0] / m[0][0];
  m[2][0] = m[2][0] / m[0][0];
#pragma unroll
  for (int c = 1; c < 4; c++) {
    m[1][c] = m[1][c] - m[1][0] * m[0][c];
    m[2][c] = m[2][c] - m[2][0] * m[0][c];
  }
  if (fabs(m[2][1]) > fabs(m[1][1])) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const double a = m[1][c];
      m[1][c] = m[2][c];
      m[2][c] = a;
    }
  }
  m[2][1] = m[2][1] / m[1][1];
  m[2][2] = m[2][2] - m[2][1] * m[1][2];
  m[2][3] = m[2][3] - m[2][1] * m[1][3];
  x[2] = m[2][3] / m[2][2];
  x[1] = (m[1][3] - m[1][2] * x[2]) / m[1][1];
  x[0] = (m[0][3] - m[0][1] * x[1] - m[0][2] * x[2]) / m[0][0];
}

// Sim3::log: omega, upsilon, sigma
__host__ __device__ inline void eg_sim3_log(const OsSim3& S, double* res) {
  const double sigma = log(S.s);
  double R[9];
  pose_rotation(S.q, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR
  const double eps = 0.00001;
  const bool small_angle = d > 1 - eps;
  double k = 0.5, theta = 0.0;
  if (!small_angle) {
    theta = acos(d);
    k = theta / (2 * sqrt(1 - d * d));
  }
  const double om[3] = {k * dR[0], k * dR[1], k * dR[2]};
  double A, B, Cc;
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
      A = ((sigma - 1) * S.s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * S.s - 1) / (sigma2 * sigma);
    } else {
      const double theta2 = theta * theta;
      const double a = S.s * sin(theta);
      const double b = S.s * cos(theta);
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (Cc - ((b - 1) * sigma + a * theta) / (c)) * 1 / (theta2);
    }
  }
  const double Om[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
  double W[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double om2 = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j];
      W[3 * i + j] = A * Om[i][j] + B * om2 + Cc * (i == j ? 1.0 : 0.0);
    }
  const double t[3] = {S.q.tx, S.q.ty, S.q.tz};
  eg_lu_solve3(W, t, res + 3);
  res[0] = om[0];
  res[1] = om[1];
  res[2] = om[2];
  res[6] = sigma;
}

// SE3Quat::log: omega, upsilon
__host__ __device__ inline void eg_se3_log(const PoseSE3& p, double* res) {
  double R[9];
  pose_rotation(p, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  double k, c2;
  if (fabs(d) > 0.99999) {
    k = 0.5;
    c2 = 1. / 12.;
  } else {
    const double theta = acos(d);
    k = theta / (2 * sqrt(1 - d * d));
    c2 = (1 - theta / (2 * tan(theta / 2))) / (theta * theta);
  }
  const double om[3] = {k * dR[0], k * dR[1], k * dR[2]};
  const double Om[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
  const double t[3] = {p.tx, p.ty, p.tz};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double V[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double om2 = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j];
      V[j] = (i == j ? 1.0 : 0.0) - 0.5 * Om[i][j] + c2 * om2;
    }
    res[3 + i] = V[0] * t[0] + V[1] * t[1] + V[2] * t[2];
  }
  res[0] = om[0];
  res[1] = om[1];
  res[2] = om[2];
}

// SE3Quat::inverse: no normalisation
__host__ __device__ inline PoseSE3 eg_se3_inverse(const PoseSE3& p) {
  PoseSE3 r;
  r.qx = -p.qx;
  r.qy = -p.qy;
  r.qz = -p.qz;
  r.qw = p.qw;
  pose_rotate(r, -p.tx, -p.ty, -p.tz, &r.tx, &r.ty, &r.tz);
  return r;
}

// EdgeSim3::computeError: (C * v1 * v2^-1).log()
__host__ __device__ inline void eg_error_sim3(const OsSim3& C, const OsSim3& Si, const OsSim3& Sj, double* e) {
  eg_sim3_log(os_mul(os_mul(C, Si), os_inverse(Sj)), e);
}

// EdgeSE3Expmap::computeError: (v2^-1 * C * v1).log()
__host__ __device__ inline void eg_error_se3(const PoseSE3& C, const PoseSE3& Ti, const PoseSE3& Tj, double* e) {
  eg_se3_log(pose_mul(pose_mul(eg_se3_inverse(Tj), C), Ti), e);
}

// sign * T.adj() into J, column-major 6 x 6: [R 0; skew(t) R  R]
__host__ __device__ inline void eg_adj(const PoseSE3& T, bool negate, double* J) {
  double R[9];
  pose_rotation(T, R);
  const double tR[9] = {-T.tz * R[3] + T.ty * R[6], -T.tz * R[4] + T.ty * R[7], -T.tz * R[5] + T.ty * R[8],
                        T.tz * R[0] - T.tx * R[6],  T.tz * R[1] - T.tx * R[7],  T.tz * R[2] - T.tx * R[8],
                        -T.ty * R[0] + T.tx * R[3], -T.ty * R[1] + T.tx * R[4], -T.ty * R[2] + T.tx * R[5]};
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double a = negate ? -R[3 * r + c] : R[3 * r + c];
      J[c * 6 + r] = a;
      J[(c + 3) * 6 + (r + 3)] = a;
      J[c * 6 + (r + 3)] = negate ? -tR[3 * r + c] : tR[3 * r + c];
      J[(c + 3) * 6 + r] = negate ? -0.0 : 0.0;
    }
}

// EdgeSE3Expmap::linearizeOplus: Ji = (Tj^-1 * Tij).adj(), Jj = -(Ti^-1 * Tij^-1).adj()
__host__ __device__ inline void eg_jacobians_se3(const PoseSE3& C, const PoseSE3& Ti, const PoseSE3& Tj, double* Ji, double* Jj) {
  eg_adj(pose_mul(eg_se3_inverse(Tj), C), false, Ji);
  eg_adj(pose_mul(eg_se3_inverse(Ti), eg_se3_inverse(C)), true, Jj);
}

// VertexSE3Expmap::oplusImpl
__host__ __device__ inline OsSim3 eg_oplus_se3(const OsSim3& T, const double* u) {
  OsSim3 r;
  r.q = pose_mul(pose_exp(u), T.q);
  r.s = 1.0;
  return r;
}

// One row of poses_out: [R | t / s] of the Sim3 path (`eigt *= (1. / s)`, Optimizer.cc:1003-1011), [R | t] of the SE3 path
__host__ __device__ inline void eg_pose_row(const OsSim3& S, bool se3, float* T) {
  double R[9];
  pose_rotation(S.q, R);
  const double k = 1. / S.s;
  T[0] = (float)R[0]; T[1] = (float)R[1]; T[2] = (float)R[2];
  T[4] = (float)R[3]; T[5] = (float)R[4]; T[6] = (float)R[5];
  T[8] = (float)R[6]; T[9] = (float)R[7]; T[10] = (float)R[8];
  T[3] = (float)(se3 ? S.q.tx : S.q.tx * k);
  T[7] = (float)(se3 ? S.q.ty : S.q.ty * k);
  T[11] = (float)(se3 ? S.q.tz : S.q.tz * k);
}

// correctedSwr.map(Srw.map(P)) with correctedSwr = CorrectedSiw.inverse() (Optimizer.cc:1002, :1030-1038); the float position
// widened, one rounding to float at the end (Converter::toCvMat)
__host__ __device__ inline void eg_correct_point(const OsSim3& from, const OsSim3& to, const float* P, float* out) {
  double x, y, z, cx, cy, cz;
  os_map(from, (double)P[0], (double)P[1], (double)P[2], &x, &y, &z);
  os_map(os_inverse(to), x, y, z, &cx, &cy, &cz);
  out[0] = (float)cx;
  out[1] = (float)cy;
  out[2] = (float)cz;
}

// ---- the workspace of one problem: doubles first, then 32-bit integers; every array sized by the caps -----------------------------
struct EgWs {
  OsSim3 *est, *bak;        // [kf_cap] the estimates and what push() saved
  OsSim3* meas;             // [edge_cap]
  double* je;               // [edge_cap][EG_EDGE_DOUBLES]
  double* env;              // [env_cap][49] the row envelope: H + lambda I, then its factor
  double *b, *y;            // [kf_cap * 7] the right-hand side; the solve's vector, at the end the update
  int32_t *cnt, *fill;      // [kf_cap] edges at a vertex
  int32_t* start;           // [kf_cap + 1] where a vertex's incidence list begins
  int32_t *slot, *kf_of_slot;   // [kf_cap] the row block of a vertex (-1: not in the system) and back
  int32_t* first;           // [kf_cap] the first row block of a row's envelope
  int32_t* row_off;         // [kf_cap + 1] blocks before a row
  int32_t* list;            // [2 * edge_cap] incidence lists: 2 * edge + (0: the vertex is i, 1: it is j), ascending
};

__host__ __device__ inline size_t eg_align(size_t b) { return (b + 255) & ~(size_t)255; }

__host__ __device__ inline size_t eg_ws_bytes(int kf_cap, int edge_cap, int env_cap) {
  const size_t k = (size_t)kf_cap, e = (size_t)edge_cap, v = (size_t)env_cap;
  return eg_align(k * 64) * 2 + eg_align(e * 64) + eg_align(e * EG_EDGE_DOUBLES * 8) + eg_align(v * 49 * 8) + eg_align(k * 56) * 2 +
         eg_align(k * 4) * 5 + eg_align((k + 1) * 4) * 2 + eg_align(e * 8);
}

__host__ __device__ inline void eg_ws_carve(uint8_t* p, int kf_cap, int edge_cap, int env_cap, EgWs& W) {
  const size_t k = (size_t)kf_cap, e = (size_t)edge_cap, v = (size_t)env_cap;
  W.est = (OsSim3*)p; p += eg_align(k * 64);
  W.bak = (OsSim3*)p; p += eg_align(k * 64);
  W.meas = (OsSim3*)p; p += eg_align(e * 64);
  W.je = (double*)p; p += eg_align(e * EG_EDGE_DOUBLES * 8);
  W.env = (double*)p; p += eg_align(v * 49 * 8);
  W.b = (double*)p; p += eg_align(k * 56);
  W.y = (double*)p; p += eg_align(k * 56);
  W.cnt = (int32_t*)p; p += eg_align(k * 4);
  W.fill = (int32_t*)p; p += eg_align(k * 4);
  W.slot = (int32_t*)p; p += eg_align(k * 4);
  W.kf_of_slot = (int32_t*)p; p += eg_align(k * 4);
  W.first = (int32_t*)p; p += eg_align(k * 4);
  W.start = (int32_t*)p; p += eg_align((k + 1) * 4);
  W.row_off = (int32_t*)p; p += eg_align((k + 1) * 4);
  W.list = (int32_t*)p;
}

struct EgLaunch {
  const orbfe_eg_problem* problems;
  const orbfe_eg_vertex* vertices;
  const orbfe_eg_edge* edges;
  int kf_cap, edge_cap, env_cap, flags;
  orbfe_eg_sim3* sim3_out;
  float* poses_out;
  orbfe_eg_result* result;
  uint8_t* workspace;
};
void orbfe_launch_essential_graph(const EgLaunch& L, int P, hipStream_t s);
void orbfe_launch_correct_points(const float* points, int n, const int32_t* ref, const uint8_t* from, int from_stride,
                                 const orbfe_eg_sim3* to, int n_tables, float* out, hipStream_t s);
