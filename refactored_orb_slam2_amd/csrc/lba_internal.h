// lba_internal.h -- the arithmetic of Optimizer::LocalBundleAdjustment, once, for the kernel (lba_kernels.hip) and for host code that
// wants the same bits (tests/cpp_lba/host_arith.cpp).  __host__ __device__ inline functions, all in double, compiled with
// -ffp-contract=off on both sides; no HIP call.  Every function here handles ONE item -- a point, an entry of a keyframe's block, an
// entry of the reduced system, an edge -- of one problem whose arrays an LbaWs names; the kernel spreads the items over its lanes,
// the host build walks them in order, and either way an item is summed by one walker in the order its list states.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/, G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o/):
//   Optimizer::LocalBundleAdjustment       L/src/Optimizer.cc:437-760
//   EdgeSE3ProjectXYZ                      G/types/sba/edge_project_xyz.cpp:51-101
//   EdgeStereoSE3ProjectXYZ                G/types/sba/edge_project_stereo_xyz.cpp:34-42, :69-115, edge_project_stereo_xyz.h:49-62
//   BaseBinaryEdge::constructQuadraticForm G/core/base_binary_edge.hpp (A: the point's block, B: the pose's)
//   BlockSolver::solve (Schur)             G/core/block_solver.hpp:332-477
//   OptimizationAlgorithmLevenberg         G/core/optimization_algorithm_levenberg.cpp:60-176 (lm_internal.h)
// SE3Quat is pose_internal.h's, the Huber kernel, the pose block's quadratic form and the trial bookkeeping are lm_internal.h's.
// Neither Eigen nor g2o can be built where this library is built: the 3 x 3 inverse is Eigen's cofactor formula written out, fixed-size
// products are taken in index order, and Eigen::SimplicialLLT with its fill-reducing ordering is a dense unpivoted L L^T of the
// reduced system in natural order.  A reading, unpinned.
//
// Edges are listed point by point, keyframes ascending inside a point, no (keyframe, point) pair twice: the order in which the
// reference adds them (Optimizer.cc:560-644) with its std::map<KeyFrame*, size_t> order read as index order.  The edges of a point
// are then one range, and the edges of a keyframe, listed in edge order, ascend in their points -- what lets an entry of the reduced
// system walk two such lists side by side.
#pragma once
#include "pose_internal.h"

constexpr int LBA_EKF = 27;   // per edge: the 21 upper entries and the 6 of b that it adds to its keyframe's block (lm_accumulate<6>)

__host__ __device__ inline double lba_bound(bool stereo) { return stereo ? 7.815 : 5.991; }   // Optimizer.cc:669, :683 (doubles)
// The Huber delta of a monocular edge in Optimizer::BundleAdjustment: (float)sqrt(5.99) (Optimizer.cc:82), where LocalBundleAdjustment
// and PoseOptimization have (float)sqrt(5.991) = pose_delta(false).  The stereo delta is pose_delta(true) in all three
__host__ __device__ inline double ba_delta_mono() { return (double)2.44744754f; }

// One problem: its inputs and its workspace
struct LbaWs {
  int n_kf, n_pt, n_e, n_free;
  const orbfe_lba_edge* edges;
  PoseIntr K;
  PoseSE3 *pose, *pose_bak;         // [n_kf]: the estimates and what push() saved
  int *slot_of_kf;                  // [n_kf]: row block of the reduced system, -1: fixed, or not active in this round
  int *kf_of_fi, *kf_start;         // [n_free], [n_free + 1]: the free keyframes and their ranges of kf_list
  int *fi_of_slot;                  // [slots]
  double *pt, *pt_bak;              // [3 n_pt]
  double *Hll, *Dinv;               // [9 n_pt]
  double *bl, *db, *xl;             // [3 n_pt]
  double *B, *Y;                    // [18 n_e]: Hpl of the edge (6 x 3), and B * Dinv of the trial
  double *Ekf;                      // [27 n_e]
  double *chi2;                     // [n_e]: what the last computeError left in the edge
  double *Hpp, *bp;                 // [21 n_free], [6 n_free]
  double *S;                        // [(6 slots)^2]: the reduced system, lower triangle, row-major
  int *pt_start, *pt_end, *kf_list; // [n_pt], [n_pt], [n_e]
  uint8_t *level, *pt_active;       // [n_e], [n_pt]
};

// The bytes of one problem's workspace for F free keyframes, NP points and NE edges, and its arrays
__host__ __device__ inline size_t lba_ws_bytes(int F, int NP, int NE) {
  const size_t d = (size_t)33 * NP + (size_t)(36 + LBA_EKF + 1) * NE + (size_t)27 * F + (size_t)36 * F * F;
  const size_t i = (size_t)2 * NP + (size_t)NE;
  const size_t b = (size_t)NE + (size_t)NP;
  return (d * 8 + i * 4 + b + 255) & ~(size_t)255;
}
__host__ __device__ inline void lba_ws_carve(uint8_t* base, int F, int NP, int NE, LbaWs& W) {
  double* d = reinterpret_cast<double*>(base);
  W.pt = d; d += (size_t)3 * NP;
  W.pt_bak = d; d += (size_t)3 * NP;
  W.Hll = d; d += (size_t)9 * NP;
  W.Dinv = d; d += (size_t)9 * NP;
  W.bl = d; d += (size_t)3 * NP;
  W.db = d; d += (size_t)3 * NP;
  W.xl = d; d += (size_t)3 * NP;
  W.B = d; d += (size_t)18 * NE;
  W.Y = d; d += (size_t)18 * NE;
  W.Ekf = d; d += (size_t)LBA_EKF * NE;
  W.chi2 = d; d += (size_t)NE;
  W.Hpp = d; d += (size_t)21 * F;
  W.bp = d; d += (size_t)6 * F;
  W.S = d; d += (size_t)36 * F * F;
  int* i = reinterpret_cast<int*>(d);
  W.pt_start = i; i += NP;
  W.pt_end = i; i += NP;
  W.kf_list = i; i += NE;
  uint8_t* b = reinterpret_cast<uint8_t*>(i);
  W.level = b; b += NE;
  W.pt_active = b;
}

// computeError + chi2() of one edge: e[3] (e[2] = 0 for a monocular edge), the camera-frame point, returns chi2.  The stereo edge's
// invz is `const double invz = 1.0f / z` here -- a double, unlike the pose-only edge's float
__host__ __device__ inline double lba_edge_error(const orbfe_lba_edge& E, const PoseIntr& K, const PoseSE3& p, double X, double Y, double Z,
                                                 double* e, double* x, double* y, double* z) {
  pose_map(p, X, Y, Z, x, y, z);
  const double w = (double)E.inv_sigma2;
  if (!(E.u_right < 0)) {
    const double invz = 1.0 / *z;
    const double r0 = *x * invz * K.fx + K.cx;
    const double r1 = *y * invz * K.fy + K.cy;
    const double r2 = r0 - K.bf * invz;
    e[0] = (double)E.u - r0;
    e[1] = (double)E.v - r1;
    e[2] = (double)E.u_right - r2;
    return e[0] * (w * e[0]) + e[1] * (w * e[1]) + e[2] * (w * e[2]);
  }
  e[0] = (double)E.u - (*x / *z * K.fx + K.cx);
  e[1] = (double)E.v - (*y / *z * K.fy + K.cy);
  e[2] = 0.0;
  return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}

// linearizeOplus of one edge at the camera-frame point (x, y, z): A (the point's rows) and B (the pose's); row 2 is the stereo edge's
__host__ __device__ inline void lba_edge_jacobians(const PoseIntr& K, const PoseSE3& p, bool stereo, double x, double y, double z,
                                                   double A[3][3], double B[3][6]) {
  double R[9];
  pose_rotation(p, R);
  const double z_2 = z * z;
  if (stereo) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      A[0][c] = -K.fx * R[c] / z + K.fx * x * R[6 + c] / z_2;
      A[1][c] = -K.fy * R[3 + c] / z + K.fy * y * R[6 + c] / z_2;
      A[2][c] = A[0][c] - K.bf * R[6 + c] / z_2;
    }
  } else {   // -1. / z * tmp * R, tmp = [[fx, 0, -x / z * fx], [0, fy, -y / z * fy]]
    const double m = -1. / z;
    const double t00 = m * K.fx, t02 = m * (-x / z * K.fx), t11 = m * K.fy, t12 = m * (-y / z * K.fy);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      A[0][c] = t00 * R[c] + t02 * R[6 + c];
      A[1][c] = t11 * R[3 + c] + t12 * R[6 + c];
      A[2][c] = 0.0;
    }
  }
  B[0][0] = x * y / z_2 * K.fx;
  B[0][1] = -(1 + (x * x / z_2)) * K.fx;
  B[0][2] = y / z * K.fx;
  B[0][3] = -1. / z * K.fx;
  B[0][4] = 0;
  B[0][5] = x / z_2 * K.fx;
  B[1][0] = (1 + y * y / z_2) * K.fy;
  B[1][1] = -x * y / z_2 * K.fy;
  B[1][2] = -x / z * K.fy;
  B[1][3] = 0;
  B[1][4] = -1. / z * K.fy;
  B[1][5] = y / z_2 * K.fy;
  B[2][0] = B[0][0] - K.bf * y / z_2;
  B[2][1] = B[0][1] + K.bf * x / z_2;
  B[2][2] = B[0][2];
  B[2][3] = B[0][3];
  B[2][4] = 0;
  B[2][5] = B[0][5] - K.bf / z_2;
}

// Eigen's inverse of a 3 x 3 matrix (row-major M[9]): the cofactors over the determinant expanded along the first column
__host__ __device__ inline void lba_inverse3(const double* M, double* R) {
  const double c00 = M[4] * M[8] - M[5] * M[7];
  const double c10 = M[7] * M[2] - M[8] * M[1];
  const double c20 = M[1] * M[5] - M[2] * M[4];
  const double det = (c00 * M[0] + c10 * M[3]) + c20 * M[6];
  const double inv = 1.0 / det;
  R[0] = c00 * inv;
  R[1] = c10 * inv;
  R[2] = c20 * inv;
  R[3] = (M[5] * M[6] - M[3] * M[8]) * inv;   // cofactor<0,1>
  R[4] = (M[8] * M[0] - M[6] * M[2]) * inv;   // <1,1>
  R[5] = (M[2] * M[3] - M[0] * M[5]) * inv;   // <2,1>
  R[6] = (M[3] * M[7] - M[4] * M[6]) * inv;   // <0,2>
  R[7] = (M[6] * M[1] - M[7] * M[0]) * inv;   // <1,2>
  R[8] = (M[0] * M[4] - M[1] * M[3]) * inv;   // <2,2>
}

// ---- building the system: one point ------------------------------------------------------------------------------------------------
// computeActiveErrors, linearizeOplus and constructQuadraticForm of the level-0 edges of point p: Hll and bl of the point, and per edge
// its chi2, its Hpl block and what it adds to its keyframe's block.  Adds the robustified chi2 to *chi and raises *maxdiag to the
// point's largest |Hll_jj|.  A point without a level-0 edge is not active.  delta_mono: the Huber delta of a monocular edge.
__host__ __device__ inline void lba_point_build(const LbaWs& W, int p, bool robust, double* chi, double* maxdiag,
                                                double delta_mono = pose_delta(false)) {
  const double X = W.pt[3 * p], Y = W.pt[3 * p + 1], Z = W.pt[3 * p + 2];
  double Hll[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
  bool any = false;
  for (int i = W.pt_start[p]; i < W.pt_end[p]; i++) {
    if (W.level[i]) continue;
    any = true;
    const orbfe_lba_edge E = W.edges[i];
    const PoseSE3 P = W.pose[E.kf];
    const bool stereo = !(E.u_right < 0);
    const double w = (double)E.inv_sigma2;
    double e[3], x, y, z, A[3][3], B[3][6];
    const double chi2 = lba_edge_error(E, W.K, P, X, Y, Z, e, &x, &y, &z);
    W.chi2[i] = chi2;
    double rho0 = chi2, rho1 = 1.0;
    if (robust) lm_huber(chi2, stereo ? pose_delta(true) : delta_mono, &rho0, &rho1);
    *chi += rho0;
    lba_edge_jacobians(W.K, P, stereo, x, y, z, A, B);
    const double ow = rho1 * w;
    const double we0 = (-(w * e[0])) * rho1, we1 = (-(w * e[1])) * rho1, we2 = (-(w * e[2])) * rho1;
    double AtO[3][3];   // [row of the edge][column of A]
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int a = 0; a < 3; a++) AtO[r][a] = A[r][a] * ow;
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
      for (int b = 0; b < 3; b++) {
        double h = AtO[0][a] * A[0][b] + AtO[1][a] * A[1][b];
        if (stereo) h = h + AtO[2][a] * A[2][b];
        Hll[3 * a + b] += h;
      }
      double g = A[0][a] * we0 + A[1][a] * we1;
      if (stereo) g = g + A[2][a] * we2;
      bl[a] += g;
    }
    if (W.slot_of_kf[E.kf] >= 0) {
      double* Be = W.B + (size_t)18 * i;
#pragma unroll
      for (int b = 0; b < 6; b++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
          double h = AtO[0][a] * B[0][b] + AtO[1][a] * B[1][b];
          if (stereo) h = h + AtO[2][a] * B[2][b];
          Be[3 * b + a] = h;
        }
      double acc[lm_nacc<6>];
#pragma unroll
      for (int k = 0; k < lm_nacc<6>; k++) acc[k] = 0.0;
      lm_accumulate<6>(B[0], B[1], B[2], stereo, e[0], e[1], e[2], w, rho0, rho1, acc);
      double* Ee = W.Ekf + (size_t)LBA_EKF * i;
#pragma unroll
      for (int k = 0; k < LBA_EKF; k++) Ee[k] = acc[k];
    }
  }
  W.pt_active[p] = any ? 1 : 0;
  if (!any) return;
#pragma unroll
  for (int k = 0; k < 9; k++) W.Hll[(size_t)9 * p + k] = Hll[k];
#pragma unroll
  for (int k = 0; k < 3; k++) W.bl[(size_t)3 * p + k] = bl[k];
  *maxdiag = fmax(fabs(Hll[0]), *maxdiag);
  *maxdiag = fmax(fabs(Hll[4]), *maxdiag);
  *maxdiag = fmax(fabs(Hll[8]), *maxdiag);
}

// Entry k (0 .. 20: upper entries of Hpp, 21 .. 26: bp) of free keyframe fi: its level-0 edges in edge order.  Returns the entry
__host__ __device__ inline double lba_kf_sum(const LbaWs& W, int fi, int k) {
  double s = 0.0;
  for (int q = W.kf_start[fi]; q < W.kf_start[fi + 1]; q++) {
    const int i = W.kf_list[q];
    if (W.level[i]) continue;
    s += W.Ekf[(size_t)LBA_EKF * i + k];
  }
  if (k < 21) W.Hpp[21 * fi + k] = s;
  else W.bp[6 * fi + (k - 21)] = s;
  return s;
}
__host__ __device__ inline bool lba_is_diag(int k) { return k == 0 || k == 6 || k == 11 || k == 15 || k == 18 || k == 20; }

// ---- one trial: the points' part of BlockSolver::solve -----------------------------------------------------------------------------
// Dinv = (Hll + lambda I)^-1, db = Dinv bl, and B Dinv of every level-0 edge of the point whose keyframe has a row block
__host__ __device__ inline void lba_point_dinv(const LbaWs& W, int p, double lambda) {
  if (!W.pt_active[p]) return;
  double M[9], D[9];
#pragma unroll
  for (int k = 0; k < 9; k++) M[k] = W.Hll[(size_t)9 * p + k];
  M[0] = M[0] + lambda;
  M[4] = M[4] + lambda;
  M[8] = M[8] + lambda;
  lba_inverse3(M, D);
  const double b0 = W.bl[3 * p], b1 = W.bl[3 * p + 1], b2 = W.bl[3 * p + 2];
#pragma unroll
  for (int k = 0; k < 9; k++) W.Dinv[(size_t)9 * p + k] = D[k];
#pragma unroll
  for (int r = 0; r < 3; r++) W.db[3 * p + r] = (D[3 * r] * b0 + D[3 * r + 1] * b1) + D[3 * r + 2] * b2;
  for (int i = W.pt_start[p]; i < W.pt_end[p]; i++) {
    if (W.level[i] || W.slot_of_kf[W.edges[i].kf] < 0) continue;
    const double* Be = W.B + (size_t)18 * i;
    double* Ye = W.Y + (size_t)18 * i;
#pragma unroll
    for (int r = 0; r < 6; r++) {
      const double a0 = Be[3 * r], a1 = Be[3 * r + 1], a2 = Be[3 * r + 2];
#pragma unroll
      for (int c = 0; c < 3; c++) Ye[3 * r + c] = (a0 * D[c] + a1 * D[3 + c]) + a2 * D[6 + c];
    }
  }
}

// Row r of bschur of free keyframe fi: bp - sum B db over its level-0 edges (the landmarks in order)
__host__ __device__ inline double lba_bschur(const LbaWs& W, int fi, int r) {
  double s = 0.0;
  for (int q = W.kf_start[fi]; q < W.kf_start[fi + 1]; q++) {
    const int i = W.kf_list[q];
    if (W.level[i]) continue;
    const double* Be = W.B + (size_t)18 * i + 3 * r;
    const double* db = W.db + (size_t)3 * W.edges[i].point;
    s += (Be[0] * db[0] + Be[1] * db[1]) + Be[2] * db[2];
  }
  return W.bp[6 * fi + r] - s;
}

// Entry (r, c) of block (fi, fj), fi <= fj, of Hschur = (Hpp + lambda I) - sum over the landmarks of (B_i Dinv) B_j^T.  For fi == fj
// only r <= c is read by the solver.  The two edge lists ascend in their points and are walked side by side
__host__ __device__ inline double lba_schur_entry(const LbaWs& W, int fi, int fj, int r, int c, double lambda) {
  double s = 0.0;
  if (fi == fj) {
    s = W.Hpp[21 * fi + lm_diag<6>(r) + (c - r)];
    if (r == c) s = s + lambda;
    for (int q = W.kf_start[fi]; q < W.kf_start[fi + 1]; q++) {
      const int i = W.kf_list[q];
      if (W.level[i]) continue;
      const double* Ye = W.Y + (size_t)18 * i + 3 * r;
      const double* Be = W.B + (size_t)18 * i + 3 * c;
      s -= (Ye[0] * Be[0] + Ye[1] * Be[1]) + Ye[2] * Be[2];
    }
    return s;
  }
  int qa = W.kf_start[fi], qb = W.kf_start[fj];
  const int ea = W.kf_start[fi + 1], eb = W.kf_start[fj + 1];
  while (qa < ea && qb < eb) {
    const int ia = W.kf_list[qa], ib = W.kf_list[qb];
    const int pa = W.edges[ia].point, pb = W.edges[ib].point;
    if (pa < pb) {
      qa++;
    } else if (pb < pa) {
      qb++;
    } else {
      if (!W.level[ia] && !W.level[ib]) {
        const double* Ye = W.Y + (size_t)18 * ia + 3 * r;
        const double* Be = W.B + (size_t)18 * ib + 3 * c;
        s -= (Ye[0] * Be[0] + Ye[1] * Be[1]) + Ye[2] * Be[2];
      }
      qa++;
      qb++;
    }
  }
  return s;
}

// The dense L L^T of the reduced system and its two triangular solves, in the order the kernel's workgroup keeps: S (lower triangle,
// row-major, n x n) is overwritten below its diagonal, the diagonal of L goes to diag; x = solution of S x = b.  false when a pivot
// is not > 0 (SimplicialLLT's info() != Success)
__host__ __device__ inline bool lba_cholesky_solve(double* S, int n, double* diag, const double* b, double* y, double* x) {
  for (int k = 0; k < n; k++) {
    const double d = S[(size_t)k * n + k];
    if (!(d > 0.0)) return false;
    const double lkk = sqrt(d);
    diag[k] = lkk;
    for (int i = k + 1; i < n; i++) S[(size_t)i * n + k] = S[(size_t)i * n + k] / lkk;
    for (int i = k + 1; i < n; i++) {
      const double lik = S[(size_t)i * n + k];
      for (int j = k + 1; j <= i; j++) S[(size_t)i * n + j] -= lik * S[(size_t)j * n + k];
    }
  }
  for (int i = 0; i < n; i++) y[i] = b[i];
  for (int k = 0; k < n; k++) {
    y[k] = y[k] / diag[k];
    for (int i = k + 1; i < n; i++) y[i] -= S[(size_t)i * n + k] * y[k];
  }
  for (int k = n - 1; k >= 0; k--) {
    y[k] = y[k] / diag[k];
    x[k] = y[k];
    for (int i = 0; i < k; i++) y[i] -= S[(size_t)k * n + i] * y[k];
  }
  return true;
}

// Back-substitution, computeScale, push and oplus of point p: cl = bl - sum B^T xp, xl = Dinv cl; xp is the poses' solution by row
// block.  Adds the point's share of computeScale to *scale
__host__ __device__ inline void lba_point_update(const LbaWs& W, int p, double lambda, const double* xp, double* scale) {
  if (!W.pt_active[p]) return;
  const double b0 = W.bl[3 * p], b1 = W.bl[3 * p + 1], b2 = W.bl[3 * p + 2];
  double c0 = b0, c1 = b1, c2 = b2;
  for (int i = W.pt_start[p]; i < W.pt_end[p]; i++) {
    if (W.level[i]) continue;
    const int slot = W.slot_of_kf[W.edges[i].kf];
    if (slot < 0) continue;
    const double* Be = W.B + (size_t)18 * i;
    const double* xs = xp + 6 * slot;
    double t0 = Be[0] * (-xs[0]), t1 = Be[1] * (-xs[0]), t2 = Be[2] * (-xs[0]);
#pragma unroll
    for (int r = 1; r < 6; r++) {
      t0 = t0 + Be[3 * r] * (-xs[r]);
      t1 = t1 + Be[3 * r + 1] * (-xs[r]);
      t2 = t2 + Be[3 * r + 2] * (-xs[r]);
    }
    c0 = c0 + t0;
    c1 = c1 + t1;
    c2 = c2 + t2;
  }
  const double* D = W.Dinv + (size_t)9 * p;
  const double x0 = (D[0] * c0 + D[1] * c1) + D[2] * c2;
  const double x1 = (D[3] * c0 + D[4] * c1) + D[5] * c2;
  const double x2 = (D[6] * c0 + D[7] * c1) + D[8] * c2;
  W.xl[3 * p] = x0;
  W.xl[3 * p + 1] = x1;
  W.xl[3 * p + 2] = x2;
  *scale += x0 * (lambda * x0 + b0);
  *scale += x1 * (lambda * x1 + b1);
  *scale += x2 * (lambda * x2 + b2);
#pragma unroll
  for (int k = 0; k < 3; k++) W.pt_bak[3 * p + k] = W.pt[3 * p + k];
  W.pt[3 * p] = W.pt[3 * p] + x0;
  W.pt[3 * p + 1] = W.pt[3 * p + 1] + x1;
  W.pt[3 * p + 2] = W.pt[3 * p + 2] + x2;
}

// The same for the keyframe of row block `slot`: push, exp(x) * estimate
__host__ __device__ inline void lba_pose_update(const LbaWs& W, int slot, double lambda, const double* xp, double* scale) {
  const int fi = W.fi_of_slot[slot], kf = W.kf_of_fi[fi];
  double x[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    x[j] = xp[6 * slot + j];
    *scale += x[j] * (lambda * x[j] + W.bp[6 * fi + j]);
  }
  const PoseSE3 P = W.pose[kf];
  W.pose_bak[kf] = P;
  W.pose[kf] = pose_mul(pose_exp(x), P);
}

// computeActiveErrors + activeRobustChi2 of the level-0 edges of point p at the estimates
__host__ __device__ inline void lba_point_chi(const LbaWs& W, int p, bool robust, double* chi, double delta_mono = pose_delta(false)) {
  if (!W.pt_active[p]) return;
  const double X = W.pt[3 * p], Y = W.pt[3 * p + 1], Z = W.pt[3 * p + 2];
  for (int i = W.pt_start[p]; i < W.pt_end[p]; i++) {
    if (W.level[i]) continue;
    const orbfe_lba_edge E = W.edges[i];
    double e[3], x, y, z;
    const double chi2 = lba_edge_error(E, W.K, W.pose[E.kf], X, Y, Z, e, &x, &y, &z);
    W.chi2[i] = chi2;
    double rho0 = chi2, rho1;
    if (robust) lm_huber(chi2, !(E.u_right < 0) ? pose_delta(true) : delta_mono, &rho0, &rho1);
    *chi += rho0;
  }
}

// pop of point p
__host__ __device__ inline void lba_point_pop(const LbaWs& W, int p) {
  if (!W.pt_active[p]) return;
#pragma unroll
  for (int k = 0; k < 3; k++) W.pt[3 * p + k] = W.pt_bak[3 * p + k];
}

// Optimizer.cc:669, :683, :707, :720: chi2() of what the last computeError left in the edge, isDepthPositive() at the estimates
__host__ __device__ inline bool lba_edge_bad(const LbaWs& W, int i) {
  const orbfe_lba_edge E = W.edges[i];
  double x, y, z;
  pose_map(W.pose[E.kf], W.pt[3 * E.point], W.pt[3 * E.point + 1], W.pt[3 * E.point + 2], &x, &y, &z);
  return W.chi2[i] > lba_bound(!(E.u_right < 0)) || !(z > 0.0);
}

// One edge of the list is acceptable where it stands: indices in range, inv_sigma2 finite and > 0, and behind its predecessor in
// (point, keyframe) order
__host__ __device__ inline bool lba_edge_valid(const orbfe_lba_edge* edges, int i, int n_kf, int n_pt) {
  const orbfe_lba_edge E = edges[i];
  if (E.kf < 0 || E.kf >= n_kf || E.point < 0 || E.point >= n_pt) return false;
  if (!(E.inv_sigma2 > 0.0f) || !isfinite(E.inv_sigma2)) return false;
  if (i > 0) {
    const orbfe_lba_edge Q = edges[i - 1];
    if (Q.point > E.point || (Q.point == E.point && Q.kf >= E.kf)) return false;
  }
  return true;
}

struct LbaLaunch {   // the arguments of orbfe_local_bundle_adjustment_batch_device
  const orbfe_pose_camera* camera;
  const orbfe_lba_problem* problems;
  const float* poses;
  const uint8_t* fixed;
  const uint8_t* points;
  int point_stride;
  const orbfe_lba_edge* edges;
  int kf_cap, point_cap, edge_cap, flags;
  float* poses_out;
  float* points_out;
  uint8_t* erase;
  orbfe_lba_result* result;
  uint8_t* workspace;
};
void orbfe_launch_lba(const LbaLaunch& L, int P, hipStream_t s);

// lba.cpp: the two entry points for either schedule of the graph.  ba: Optimizer::BundleAdjustment -- ONE optimize(n_iterations),
// d_result / result is an orbfe_ba_result and no erase list exists (erase may be null); otherwise LocalBundleAdjustment's two rounds
struct LbaSchedule {
  const char* who;   // the name error messages carry
  int n_iterations;  // read iff ba
  int known_flags;
  bool ba = false;
};
int lba_batch_entry(const LbaSchedule& S, int P, const orbfe_pose_camera* d_camera, const orbfe_lba_problem* d_problems,
                    const float* d_poses, const uint8_t* d_fixed, const uint8_t* d_points, int point_stride, const orbfe_lba_edge* d_edges,
                    int kf_cap, int point_cap, int edge_cap, int flags, float* d_poses_out, float* d_points_out, uint8_t* d_erase,
                    void* d_result, void* d_workspace, size_t workspace_bytes, void* stream);
int lba_host_entry(const LbaSchedule& S, const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf,
                   const float* points, int n_points, const orbfe_lba_edge* edges, int n_edges, int flags, float* poses_out,
                   float* points_out, uint8_t* erase, void* result);
// ba_kernels.hip: the same arguments under Optimizer::BundleAdjustment's schedule; L.flags holds ORBFE_BA_*, L.erase and L.result are not read
void orbfe_launch_ba(const LbaLaunch& L, int n_iterations, orbfe_ba_result* result, int P, hipStream_t s);
