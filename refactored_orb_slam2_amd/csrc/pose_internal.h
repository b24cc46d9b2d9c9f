// pose_internal.h -- the arithmetic of Optimizer::PoseOptimization, once, for the kernel (pose_kernels.hip) and for host code that
// wants the same bits.  __host__ __device__ inline functions, all in double, compiled with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/, G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o/):
//   Optimizer::PoseOptimization            L/src/Optimizer.cc:233-435
//   Converter::toSE3Quat / toCvMat         L/src/Converter.cc:36-46, :48-70
//   EdgeSE3ProjectXYZOnlyPose              G/types/sba/edge_project_xyz_onlypose.cpp:59-95
//   EdgeStereoSE3ProjectXYZOnlyPose        G/types/sba/edge_project_stereo_xyz_onlypose.cpp:59-109
//   SE3Quat (map, exp, operator*)          G/types/slam3d/se3quat.h:53-56, :97-103, :200-230, :251-256
//   VertexSE3Expmap::oplusImpl             G/types/sba/vertex_se3_expmap.cpp:48-51
// The Huber kernel, the quadratic form, the Levenberg bookkeeping and the dense solve are lm_internal.h's, for a vertex of 6 dimensions.
// Neither Eigen nor g2o can be built where this library is built: the quaternion formulas are Eigen's (Quaternion(Matrix3),
// toRotationMatrix, _transformVector, operator*) and fixed-size products are taken in index order.  A reading, unpinned (DESIGN
// section 2).  theta^3 of SE3Quat::exp is theta * theta * theta, not pow(theta, 3).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/orbfe.h"
#include "lm_internal.h"

constexpr int POSE_NACC = lm_nacc<6>;   // 21 upper entries of H, 6 of b, chi

struct PoseSE3 {   // g2o::SE3Quat: unit quaternion (w >= 0) and translation
  double qx, qy, qz, qw;
  double tx, ty, tz;
};

struct PoseIntr {   // fx .. bf of the edges: the Frame's floats widened (L/src/Optimizer.cc:300-303, :338-342)
  double fx, fy, cx, cy, bf;
};

// (float)sqrt(5.991), (float)sqrt(7.815) (Optimizer.cc:269-270) and the float bounds of :363-364
__host__ __device__ inline double pose_delta(bool stereo) { return stereo ? (double)2.79553223f : (double)2.44765186f; }
__host__ __device__ inline float pose_bound(bool stereo) { return stereo ? 7.815f : 5.991f; }

// SE3Quat::normalizeRotation
__host__ __device__ inline void pose_normalize(PoseSE3& p) {
  if (p.qw < 0) {
    p.qx = -p.qx;
    p.qy = -p.qy;
    p.qz = -p.qz;
    p.qw = -p.qw;
  }
  const double n = sqrt(p.qx * p.qx + p.qy * p.qy + p.qz * p.qz + p.qw * p.qw);
  p.qx = p.qx / n;
  p.qy = p.qy / n;
  p.qz = p.qz / n;
  p.qw = p.qw / n;
}

// Eigen::Quaternion(Matrix3); the three cases of the trace <= 0 branch are written out (no run-time index)
__host__ __device__ inline void pose_quat_from_matrix(double m00, double m01, double m02, double m10, double m11, double m12,
                                                      double m20, double m21, double m22, PoseSE3& p) {
  double t = m00 + m11 + m22;
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    p.qw = 0.5 * t;
    t = 0.5 / t;
    p.qx = (m21 - m12) * t;
    p.qy = (m02 - m20) * t;
    p.qz = (m10 - m01) * t;
  } else if (!(m11 > m00) && !(m22 > m00)) {   // i = 0, j = 1, k = 2
    t = sqrt(m00 - m11 - m22 + 1.0);
    p.qx = 0.5 * t;
    t = 0.5 / t;
    p.qw = (m21 - m12) * t;
    p.qy = (m10 + m01) * t;
    p.qz = (m20 + m02) * t;
  } else if (m11 > m00 && !(m22 > m11)) {      // i = 1, j = 2, k = 0
    t = sqrt(m11 - m22 - m00 + 1.0);
    p.qy = 0.5 * t;
    t = 0.5 / t;
    p.qw = (m02 - m20) * t;
    p.qz = (m21 + m12) * t;
    p.qx = (m01 + m10) * t;
  } else {                                     // i = 2, j = 0, k = 1
    t = sqrt(m22 - m00 - m11 + 1.0);
    p.qz = 0.5 * t;
    t = 0.5 / t;
    p.qw = (m10 - m01) * t;
    p.qx = (m02 + m20) * t;
    p.qy = (m12 + m21) * t;
  }
}

// Converter::toSE3Quat of the float pose (12 floats: rows of [R | t])
__host__ __device__ inline PoseSE3 pose_from_Tcw(const float* T) {
  PoseSE3 p;
  pose_quat_from_matrix((double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9],
                        (double)T[10], p);
  p.tx = (double)T[3];
  p.ty = (double)T[7];
  p.tz = (double)T[11];
  pose_normalize(p);
  return p;
}

// Eigen toRotationMatrix of the pose's quaternion, row-major with `stride` elements from row to row, each entry stored as a double or
// rounded to float.  With `translation` the rows are those of [R | t].  The statements stand in the order of the stores: a caller's
// listing depends on it.
template <class T>
__host__ __device__ inline void pose_rotation(const PoseSE3& p, T* R, int stride = 3, bool translation = false) {
  const double tx = 2.0 * p.qx, ty = 2.0 * p.qy, tz = 2.0 * p.qz;
  const double twx = tx * p.qw, twy = ty * p.qw, twz = tz * p.qw;
  const double txx = tx * p.qx, txy = ty * p.qx, txz = tz * p.qx;
  const double tyy = ty * p.qy, tyz = tz * p.qy, tzz = tz * p.qz;
  R[0] = (T)(1.0 - (tyy + tzz));
  R[1] = (T)(txy - twz);
  R[2] = (T)(txz + twy);
  if (translation) R[3] = (T)p.tx;
  R[stride] = (T)(txy + twz);
  R[stride + 1] = (T)(1.0 - (txx + tzz));
  R[stride + 2] = (T)(tyz - twx);
  if (translation) R[stride + 3] = (T)p.ty;
  R[2 * stride] = (T)(txz - twy);
  R[2 * stride + 1] = (T)(tyz + twx);
  R[2 * stride + 2] = (T)(1.0 - (txx + tyy));
  if (translation) R[2 * stride + 3] = (T)p.tz;
}

// Converter::toCvMat(SE3Quat): to_homogeneous_matrix, double -> float: the 12 floats of [R | t]
__host__ __device__ inline void pose_to_Tcw(const PoseSE3& p, float* T) { pose_rotation(p, T, 4, true); }

// Eigen _transformVector: uv = q.vec x v; uv += uv; v + w uv + q.vec x uv
__host__ __device__ inline void pose_rotate(const PoseSE3& p, double vx, double vy, double vz, double* ox, double* oy, double* oz) {
  double ux = p.qy * vz - p.qz * vy;
  double uy = p.qz * vx - p.qx * vz;
  double uz = p.qx * vy - p.qy * vx;
  ux = ux + ux;
  uy = uy + uy;
  uz = uz + uz;
  *ox = vx + p.qw * ux + (p.qy * uz - p.qz * uy);
  *oy = vy + p.qw * uy + (p.qz * ux - p.qx * uz);
  *oz = vz + p.qw * uz + (p.qx * uy - p.qy * ux);
}

// SE3Quat::map
__host__ __device__ inline void pose_map(const PoseSE3& p, double X, double Y, double Z, double* x, double* y, double* z) {
  double rx, ry, rz;
  pose_rotate(p, X, Y, Z, &rx, &ry, &rz);
  *x = rx + p.tx;
  *y = ry + p.ty;
  *z = rz + p.tz;
}

// SE3Quat::operator*
__host__ __device__ inline PoseSE3 pose_mul(const PoseSE3& a, const PoseSE3& b) {
  PoseSE3 r;
  double rx, ry, rz;
  pose_rotate(a, b.tx, b.ty, b.tz, &rx, &ry, &rz);
  r.tx = a.tx + rx;
  r.ty = a.ty + ry;
  r.tz = a.tz + rz;
  r.qx = a.qw * b.qx + a.qx * b.qw + a.qy * b.qz - a.qz * b.qy;
  r.qy = a.qw * b.qy + a.qy * b.qw + a.qz * b.qx - a.qx * b.qz;
  r.qz = a.qw * b.qz + a.qz * b.qw + a.qx * b.qy - a.qy * b.qx;
  r.qw = a.qw * b.qw - a.qx * b.qx - a.qy * b.qy - a.qz * b.qz;
  pose_normalize(r);
  return r;
}

// SE3Quat::exp of (omega, upsilon)
__host__ __device__ inline PoseSE3 pose_exp(const double* u) {
  const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double Om[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
  double Om2[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Om2[i][j] = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j];
  double a, b, d;
  if (theta < 0.00001) {
    a = 1.0;
    b = 0.5;
    d = 1.0 / 6.0;
  } else {
    const double s = sin(theta), c = cos(theta);
    a = s / theta;
    b = (1 - c) / (theta * theta);
    d = (theta - s) / (theta * theta * theta);
  }
  double R[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double eye = i == j ? 1.0 : 0.0;
      R[i][j] = eye + a * Om[i][j] + b * Om2[i][j];
      V[i][j] = eye + b * Om[i][j] + d * Om2[i][j];
    }
  PoseSE3 p;
  pose_quat_from_matrix(R[0][0], R[0][1], R[0][2], R[1][0], R[1][1], R[1][2], R[2][0], R[2][1], R[2][2], p);
  p.tx = V[0][0] * u[3] + V[0][1] * u[4] + V[0][2] * u[5];
  p.ty = V[1][0] * u[3] + V[1][1] * u[4] + V[1][2] * u[5];
  p.tz = V[2][0] * u[3] + V[2][1] * u[4] + V[2][2] * u[5];
  pose_normalize(p);
  return p;
}

// One edge as the optimiser holds it: the observation and Xw are the Frame's / the MapPoint's floats widened, w = mvInvLevelSigma2
struct PoseEdge {
  double ou, ov, our;   // mvKeysUn[i].pt, mvuRight[i]
  double X, Y, Z;       // GetWorldPos()
  double w;             // information = w * I
  bool stereo;          // !(mvuRight[i] < 0)
};

// computeError + chi2() at pose p: e[3] (e[2] = 0 for a monocular edge), the camera-frame point, returns chi2
__host__ __device__ inline double pose_edge_error(const PoseEdge& E, const PoseIntr& K, const PoseSE3& p, double* e, double* x, double* y,
                                                  double* z) {
  pose_map(p, E.X, E.Y, E.Z, x, y, z);
  if (E.stereo) {
    const float invz = (float)(1.0 / *z);   // `const float invz = 1.0f / trans_xyz[2]`: a double quotient stored in a float
    const double r0 = *x * invz * K.fx + K.cx;
    const double r1 = *y * invz * K.fy + K.cy;
    const double r2 = r0 - K.bf * invz;
    e[0] = E.ou - r0;
    e[1] = E.ov - r1;
    e[2] = E.our - r2;
    return e[0] * (E.w * e[0]) + e[1] * (E.w * e[1]) + e[2] * (E.w * e[2]);
  }
  e[0] = E.ou - (*x / *z * K.fx + K.cx);
  e[1] = E.ov - (*y / *z * K.fy + K.cy);
  e[2] = 0.0;
  return e[0] * (E.w * e[0]) + e[1] * (E.w * e[1]);
}

// linearizeOplus of one edge at the camera-frame point (x, y, z): the rows of its Jacobian (J2: the stereo edge's third), which the
// caller hands to lm_accumulate<6> with E.stereo, e, E.w and the robust kernel's rho
__host__ __device__ inline void pose_edge_jacobian(const PoseIntr& K, double x, double y, double z, double* J0, double* J1, double* J2) {
  const double invz = 1.0 / z;
  const double invz_2 = invz * invz;
  J0[0] = x * y * invz_2 * K.fx;
  J0[1] = -(1 + (x * x * invz_2)) * K.fx;
  J0[2] = y * invz * K.fx;
  J0[3] = -invz * K.fx;
  J0[4] = 0;
  J0[5] = x * invz_2 * K.fx;
  J1[0] = (1 + y * y * invz_2) * K.fy;
  J1[1] = -x * y * invz_2 * K.fy;
  J1[2] = -x * invz * K.fy;
  J1[3] = 0;
  J1[4] = -invz * K.fy;
  J1[5] = y * invz_2 * K.fy;
  J2[0] = J0[0] - K.bf * y * invz_2;
  J2[1] = J0[1] + K.bf * x * invz_2;
  J2[2] = J0[2];
  J2[3] = J0[3];
  J2[4] = 0;
  J2[5] = J0[5] - K.bf * invz_2;
}

void orbfe_launch_pose_optimize(int n_frames, const orbfe_keypoint* keys_un, const float* u_right, const int32_t* n, int cap,
                                int32_t* assigned, const uint8_t* points, int point_stride, const int32_t* n_points, int p_cap,
                                int frame_shift, const orbfe_pose_camera* camera, const float* Tcw_in, orbfe_pose_result* result,
                                uint8_t* outlier, int flags, hipStream_t s);
