// pnp_internal.h -- the arithmetic of PnPsolver, once, for the kernels (pnp_kernels.hip) and for host code that wants the same
// bits (tests/cpp_pnp/host_arith.cpp).  __host__ __device__ inline functions, compiled with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   CheckInliers                                     L/src/PnPsolver.cc:291-320
//   choose_control_points / barycentric coordinates  L/src/PnPsolver.cc:355-410
//   fill_M, compute_pose                             L/src/PnPsolver.cc:412-500
//   estimate_R_and_t, solve_for_sign                 L/src/PnPsolver.cc:538-627
//   find_betas_approx_{1,2,3}, compute_L_6x10, rho   L/src/PnPsolver.cc:632-772
//   gauss_newton, qr_solve                           L/src/PnPsolver.cc:774-908
// All of compute_pose is double; CheckInliers rounds Xc, Yc, invZc, distX, distY and error2 to float and keeps ue, ve in double.
//
// One solve is the work of `nl` cooperating lanes that share a PnpWork: nl == 64 lanes of one wave with the PnpWork in LDS on the
// device, nl == 1 on the host.  Every function below is called by all nl lanes with the same arguments but `lane`; a loop written
// `for (e = lane; e < E; e += nl)` distributes independent items, a block under `if (lane == 0)` is one lane's, and PNP_SYNC()
// separates a phase that writes the PnpWork from one that reads it.  An item's arithmetic does not depend on the lane that runs
// it, so both sides compute the same bits.
//
// The legacy CvMat routines are not available where this library is built:
//   cvSVD of a symmetric matrix (PW0tPW0, MtM)   cyclic two-sided Jacobi in double: jacobi_twosided_mem for the 3x3, pnp_jacobi12 for
//                                                 the 12x12 (each of the 11 rounds of a sweep rotates six disjoint pairs in the
//                                                 round-robin order, spread over the lanes); eigenvalues ordered by magnitude
//   cvInvert(CV_SVD) 3x3, cvSolve(CV_SVD) 6xk,   one-sided (Hestenes) Jacobi on the columns (jacobi_onesided_mem), A = W V^T, orthogonal w_j:
//   cvSVD of ABt                                  A^+ = V diag(1 / |w_j|^2) W^T, U V^T = sum_j (w_j / |w_j|) v_j^T.  On a full-column-
//                                                 rank matrix that is the unique least-squares solution.  There is no threshold: a
//                                                 zero singular value is 0 / 0 and what follows is NaN (a coplanar set).
// Non-finite values: every comparison that decides a rotation is written `!(x > y)` so that NaN means "do not rotate", and every
// loop has a fixed bound or a sweep cap; nothing can loop or trap on a NaN.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/orbfe.h"
#include "jacobi_internal.h"

#define PNP_HD __host__ __device__ __forceinline__
#define PNP_EPS 0x1p-53   // both convergence tests; the 12x12 converges in 8-12 sweeps, the small ones in 4-6

#if defined(__HIP_DEVICE_COMPILE__)
// the lanes of one wave: LDS operations of a wave complete in order, the fences keep the compiler from moving them
#define PNP_SYNC()                                           \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
    __builtin_amdgcn_wave_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
  } while (0)
#else
#define PNP_SYNC() do { } while (0)
#endif

struct PnpStart {          // one of the three starts of compute_pose (:479-489)
  double betas[4], R[9], t[3], err;
  double W[30], Vk[25];    // the 6 x k system / the 3 x 3 ABt and its right rotations
  double d[6], x5[5];      // (w_j . rho) / |w_j|^2, the least-squares solution
  double ga[24], gb[6], gx[4], A1[4], A2[4];   // gauss_newton's A, b, x and qr_solve's two vectors
  double ccs[12];
};
struct PnpWork {
  double A[144], V[144];   // MtM and the accumulated rotations (eigenvectors in columns)
  double cs[12];           // c, s of the six rotations of a round
  double cws[12], ci[9];   // control points, CC_inv
  double Vs[48], eig[5];   // v[0..3] as rows, their eigenvalues and the fifth
  double L[60], rho[6];
  double S[9], SV[9];      // 3 x 3 workspace of the PCA and of the inverse
  PnpStart st[3];
  int32_t rot, ord[12], pad[3];
};
struct PnpCamera { double fu, fv, uc, vc; };

// true when (i0 .. i3) can be a draw of :187-197: inside [0, n) and pairwise different
PNP_HD bool pnp_set_ok(int i0, int i1, int i2, int i3, int n) {
  return i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n && i3 >= 0 && i3 < n && i0 != i1 && i0 != i2 && i0 != i3 && i1 != i2 &&
         i1 != i3 && i2 != i3;
}

// CheckInliers for one correspondence (:295-313)
PNP_HD bool pnp_is_inlier(const double* R, const double* t, const PnpCamera& K, const orbfe_pnp_point& p, float* error2_out) {
  const double x = p.Xw[0], y = p.Xw[1], z = p.Xw[2];
  const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
  const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
  const float invZc = (float)(1 / (R[6] * x + R[7] * y + R[8] * z + t[2]));
  const double ue = K.uc + K.fu * Xc * invZc;
  const double ve = K.vc + K.fv * Yc * invZc;
  const float distX = (float)(p.u - ue);
  const float distY = (float)(p.v - ve);
  const float error2 = distX * distX + distY * distY;
  if (error2_out) *error2_out = error2;
  return error2 < p.max_err;
}

// the pair j (0..5) of round r (0..10) of the round-robin order on 12 indices: index 11 stays, the others turn
PNP_HD void pnp_round_pair(int r, int j, int& p, int& q) {
  int a, b;
  if (j == 0) { a = 11; b = r; }
  else { a = (r + j) % 11; b = (r + 11 - j) % 11; }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// cyclic two-sided Jacobi of the symmetric 12 x 12 w->A by all lanes; w->V receives the eigenvectors in its columns
PNP_HD void pnp_jacobi12(PnpWork* w, int lane, int nl) {
  double* A = w->A;
  double* V = w->V;
  for (int e = lane; e < 144; e += nl) V[e] = (e / 12 == e % 12) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
    if (lane == 0) w->rot = 0;
    PNP_SYNC();
    for (int r = 0; r < 11; r++) {
      for (int j = lane; j < 6; j += nl) {
        int p, q;
        pnp_round_pair(r, j, p, q);
        const double apq = A[p * 12 + q], app = A[p * 12 + p], aqq = A[q * 12 + q];
        double t, c = 1.0, s = 0.0;
        if (!jacobi_diagonal(app, aqq, apq, PNP_EPS)) {
          jacobi_rotation(app, aqq, apq, t, c, s);
          w->rot = 1;
        }
        w->cs[2 * j] = c; w->cs[2 * j + 1] = s;
      }
      PNP_SYNC();
      for (int e = lane; e < 72; e += nl) {   // A <- A J, V <- V J: columns p and q of row k
        const int j = e / 12, k = e % 12;
        const double c = w->cs[2 * j], s = w->cs[2 * j + 1];
        if (s == 0.0) continue;
        int p, q;
        pnp_round_pair(r, j, p, q);
        double x = A[k * 12 + p], y = A[k * 12 + q];
        A[k * 12 + p] = c * x - s * y; A[k * 12 + q] = s * x + c * y;
        x = V[k * 12 + p]; y = V[k * 12 + q];
        V[k * 12 + p] = c * x - s * y; V[k * 12 + q] = s * x + c * y;
      }
      PNP_SYNC();
      for (int e = lane; e < 72; e += nl) {   // A <- J^T A: rows p and q of column k
        const int j = e / 12, k = e % 12;
        const double c = w->cs[2 * j], s = w->cs[2 * j + 1];
        if (s == 0.0) continue;
        int p, q;
        pnp_round_pair(r, j, p, q);
        const double x = A[p * 12 + k], y = A[q * 12 + k];
        A[p * 12 + k] = k == q ? 0.0 : c * x - s * y;
        A[q * 12 + k] = k == p ? 0.0 : s * x + c * y;
      }
      PNP_SYNC();
    }
    if (!w->rot) break;   // uniform: every lane reads the same word
    PNP_SYNC();
  }
}

PNP_HD void pnp_alphas(const PnpWork* w, const orbfe_pnp_point& pt, double* a) {   // :400-409
  const double* ci = w->ci;
  const double d0 = (double)pt.Xw[0] - w->cws[0], d1 = (double)pt.Xw[1] - w->cws[1], d2 = (double)pt.Xw[2] - w->cws[2];
#pragma unroll
  for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
  a[0] = 1.0 - a[1] - a[2] - a[3];
}

// choose_control_points and compute_barycentric_coordinates up to CC_inv (:355-398); one lane
PNP_HD void pnp_control_points(PnpWork* w, const orbfe_pnp_point* pts, const int32_t* sel, int m) {
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  for (int i = 0; i < m; i++) {
    const orbfe_pnp_point& p = pts[sel[i]];
    c0 += (double)p.Xw[0]; c1 += (double)p.Xw[1]; c2 += (double)p.Xw[2];
  }
  c0 /= m; c1 /= m; c2 /= m;
  w->cws[0] = c0; w->cws[1] = c1; w->cws[2] = c2;
  double s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
  for (int i = 0; i < m; i++) {
    const orbfe_pnp_point& p = pts[sel[i]];
    const double x = (double)p.Xw[0] - c0, y = (double)p.Xw[1] - c1, z = (double)p.Xw[2] - c2;
    s00 += x * x; s01 += x * y; s02 += x * z; s11 += y * y; s12 += y * z; s22 += z * z;
  }
  double* S = w->S;
  S[0] = s00; S[1] = s01; S[2] = s02; S[3] = s01; S[4] = s11; S[5] = s12; S[6] = s02; S[7] = s12; S[8] = s22;
  jacobi_twosided_mem(S, w->SV, 3, PNP_EPS, JACOBI_SWEEPS);
  // dc descending, uct rows = the eigenvectors (cvSVD orders singular values, i.e. magnitudes)
  int o0 = 0, o1 = 1, o2 = 2, x;
  if (fabs(S[4 * o1]) > fabs(S[4 * o0])) { x = o0; o0 = o1; o1 = x; }
  if (fabs(S[4 * o2]) > fabs(S[4 * o1])) { x = o1; o1 = o2; o2 = x; }
  if (fabs(S[4 * o1]) > fabs(S[4 * o0])) { x = o0; o0 = o1; o1 = x; }
  w->ord[0] = o0; w->ord[1] = o1; w->ord[2] = o2;
  for (int i = 1; i < 4; i++) {
    const int o = w->ord[i - 1];
    const double k = sqrt(S[4 * o] / m);
    for (int j = 0; j < 3; j++) w->cws[3 * i + j] = w->cws[j] + k * w->SV[3 * j + o];
  }
  // CC (:394-396), its inverse through A^+ = V diag(1 / |w_j|^2) W^T
  for (int i = 0; i < 3; i++)
    for (int j = 1; j < 4; j++) S[3 * i + j - 1] = w->cws[3 * j + i] - w->cws[i];
  jacobi_onesided_mem(S, w->SV, 3, 3, PNP_EPS, JACOBI_SWEEPS);
  double inv[3];
#pragma unroll
  for (int j = 0; j < 3; j++) inv[j] = 1.0 / (S[j] * S[j] + S[3 + j] * S[3 + j] + S[6 + j] * S[6 + j]);
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++)
      w->ci[3 * a + b] = w->SV[3 * a] * (S[3 * b] * inv[0]) + w->SV[3 * a + 1] * (S[3 * b + 1] * inv[1]) + w->SV[3 * a + 2] * (S[3 * b + 2] * inv[2]);
}

// entry (ca, cb) of MtM (:412-426, :465): the rows of M in order, two per correspondence
PNP_HD double pnp_mtm_entry(const PnpWork* w, const PnpCamera& K, const orbfe_pnp_point* pts, const int32_t* sel, int m, int ca, int cb) {
  const int ia = ca / 3, ka = ca % 3, ib = cb / 3, kb = cb % 3;
  double acc = 0.0;
  for (int i = 0; i < m; i++) {
    const orbfe_pnp_point& p = pts[sel[i]];
    double a[4];
    pnp_alphas(w, p, a);
    const double aa = ia == 0 ? a[0] : ia == 1 ? a[1] : ia == 2 ? a[2] : a[3];
    const double ab = ib == 0 ? a[0] : ib == 1 ? a[1] : ib == 2 ? a[2] : a[3];
    const double du = K.uc - (double)p.u, dv = K.vc - (double)p.v;
    const double m1a = ka == 0 ? aa * K.fu : ka == 1 ? 0.0 : aa * du, m2a = ka == 0 ? 0.0 : ka == 1 ? aa * K.fv : aa * dv;
    const double m1b = kb == 0 ? ab * K.fu : kb == 1 ? 0.0 : ab * du, m2b = kb == 0 ? 0.0 : kb == 1 ? ab * K.fv : ab * dv;
    acc += m1a * m1b;
    acc += m2a * m2b;
  }
  return acc;
}

// qr_solve (:818-908) on the 6 x 4 A, read literally: the pivot search never looks at the last row, and the eta == 0 exit leaves x
PNP_HD void pnp_qr_solve(double* A, double* b, double* X, double* A1, double* A2) {
  const int nr = 6, nc = 4;
  for (int k = 0; k < nc; k++) {
    double eta = fabs(A[k * nc + k]);
    for (int i = k + 1; i < nr; i++) {
      const double elt = fabs(A[(i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) {
      A1[k] = A2[k] = 0.0;
      return;
    }
    double sum = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < nr; i++) {
      A[i * nc + k] *= inv_eta;
      sum += A[i * nc + k] * A[i * nc + k];
    }
    double sigma = sqrt(sum);
    if (A[k * nc + k] < 0) sigma = -sigma;
    A[k * nc + k] += sigma;
    A1[k] = sigma * A[k * nc + k];
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; j++) {
      double sum2 = 0;
      for (int i = k; i < nr; i++) sum2 += A[i * nc + k] * A[i * nc + j];
      const double tau = sum2 / A1[k];
      for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
    }
  }
  for (int j = 0; j < nc; j++) {   // b <- Qt b
    double tau = 0;
    for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
    tau /= A1[j];
    for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
  }
  X[nc - 1] = b[nc - 1] / A2[nc - 1];   // X = R-1 b
  for (int i = nc - 2; i >= 0; i--) {
    double sum = 0;
    for (int j = i + 1; j < nc; j++) sum += A[i * nc + j] * X[j];
    X[i] = (b[i] - sum) / A2[i];
  }
}

// one start: find_betas_approx_{s+1}, gauss_newton, compute_R_and_t (:479-489); one lane per start
PNP_HD void pnp_start(PnpWork* w, const PnpCamera& K, const orbfe_pnp_point* pts, const int32_t* sel, int m, int s) {
  PnpStart& T = w->st[s];
  const double* L = w->L;
  const double* rho = w->rho;
  const int k = s == 0 ? 4 : s == 1 ? 3 : 5;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < k; j++) {
      const int col = s == 0 ? (j == 0 ? 0 : j == 1 ? 1 : j == 2 ? 3 : 6) : j;   // :639-642, :670-672, :702-706
      T.W[i * k + j] = L[10 * i + col];
    }
  jacobi_onesided_mem(T.W, T.Vk, 6, k, PNP_EPS, JACOBI_SWEEPS);
  for (int j = 0; j < k; j++) {
    double wr = 0.0, ww = 0.0;
    for (int r = 0; r < 6; r++) {
      wr += T.W[r * k + j] * rho[r];
      ww += T.W[r * k + j] * T.W[r * k + j];
    }
    T.d[j] = wr / ww;
  }
  for (int a = 0; a < k; a++) {
    double x = 0.0;
    for (int j = 0; j < k; j++) x += T.Vk[a * k + j] * T.d[j];
    T.x5[a] = x;
  }
  double* betas = T.betas;
  const double* b = T.x5;
  if (s == 0) {          // :647-657
    if (b[0] < 0) {
      betas[0] = sqrt(-b[0]); betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0];
    } else {
      betas[0] = sqrt(b[0]); betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0];
    }
  } else {               // :677-689, :711-721
    if (b[0] < 0) {
      betas[0] = sqrt(-b[0]);
      betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
    } else {
      betas[0] = sqrt(b[0]);
      betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = s == 1 ? 0.0 : b[3] / betas[0];
    betas[3] = 0.0;
  }
  // gauss_newton (:800-816)
  for (int i = 0; i < 4; i++) T.gx[i] = 0.0;
  for (int it = 0; it < 5; it++) {
    // The ten columns of L are the products B_ab = beta_a beta_b, a <= b, at column b (b + 1) / 2 + a (:629).  Row i of the system
    // (:774-798): the residual rho_i - sum L_i[ab] beta_a beta_b in column order, and its derivative by beta_c, sum over a of
    // L_i[ac] beta_a with the square term doubled, in the order a = 0 .. 3.
    for (int i = 0; i < 6; i++) {
      const double* Li = L + 10 * i;
      for (int c = 0; c < 4; c++) {
        double g = 0.0;
        for (int a = 0; a < 4; a++) {
          const int lo = a < c ? a : c, hi = a < c ? c : a;
          const double l = Li[hi * (hi + 1) / 2 + lo];
          const double term = (a == c ? 2 * l : l) * betas[a];
          g = a == 0 ? term : g + term;
        }
        T.ga[4 * i + c] = g;
      }
      double q = 0.0;
      for (int hi = 0; hi < 4; hi++)
        for (int lo = 0; lo <= hi; lo++) {
          const double term = Li[hi * (hi + 1) / 2 + lo] * betas[lo] * betas[hi];
          q = (hi == 0) ? term : q + term;
        }
      T.gb[i] = rho[i] - q;
    }
    pnp_qr_solve(T.ga, T.gb, T.gx, T.A1, T.A2);
    for (int i = 0; i < 4; i++) betas[i] += T.gx[i];
  }
  // compute_R_and_t (:617-627): compute_ccs, compute_pcs, solve_for_sign on the first point, estimate_R_and_t, reprojection_error
  for (int e = 0; e < 12; e++) {
    double c = 0.0;
    for (int i = 0; i < 4; i++) c += betas[i] * w->Vs[12 * i + e];
    T.ccs[e] = c;
  }
  {
    double a[4];
    pnp_alphas(w, pts[sel[0]], a);
    const double z0 = a[0] * T.ccs[2] + a[1] * T.ccs[5] + a[2] * T.ccs[8] + a[3] * T.ccs[11];
    if (z0 < 0.0)
      for (int e = 0; e < 12; e++) T.ccs[e] = -T.ccs[e];
  }
  const double* cc = T.ccs;
  double pc0[3] = {0.0, 0.0, 0.0}, pw0[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < m; i++) {
    const orbfe_pnp_point& p = pts[sel[i]];
    double a[4];
    pnp_alphas(w, p, a);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      pc0[j] += a[0] * cc[j] + a[1] * cc[3 + j] + a[2] * cc[6 + j] + a[3] * cc[9 + j];
      pw0[j] += (double)p.Xw[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 3; j++) { pc0[j] /= m; pw0[j] /= m; }
  double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < m; i++) {
    const orbfe_pnp_point& p = pts[sel[i]];
    double a[4];
    pnp_alphas(w, p, a);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double pcj = a[0] * cc[j] + a[1] * cc[3 + j] + a[2] * cc[6 + j] + a[3] * cc[9 + j];
      abt[3 * j] += (pcj - pc0[j]) * ((double)p.Xw[0] - pw0[0]);
      abt[3 * j + 1] += (pcj - pc0[j]) * ((double)p.Xw[1] - pw0[1]);
      abt[3 * j + 2] += (pcj - pc0[j]) * ((double)p.Xw[2] - pw0[2]);
    }
  }
#pragma unroll
  for (int e = 0; e < 9; e++) T.W[e] = abt[e];
  jacobi_onesided_mem(T.W, T.Vk, 3, 3, PNP_EPS, JACOBI_SWEEPS);   // ABt = W V^T; R = U V^T (:578-580)
  double is[3];
#pragma unroll
  for (int j = 0; j < 3; j++) is[j] = 1.0 / sqrt(T.W[j] * T.W[j] + T.W[3 + j] * T.W[3 + j] + T.W[6 + j] * T.W[6 + j]);
  double R[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      R[3 * i + j] = (T.W[3 * i] * is[0]) * T.Vk[3 * j] + (T.W[3 * i + 1] * is[1]) * T.Vk[3 * j + 1] + (T.W[3 * i + 2] * is[2]) * T.Vk[3 * j + 2];
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
  if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }   // row 2, as written (:586-590)
  double t[3];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = pc0[i] - (R[3 * i] * pw0[0] + R[3 * i + 1] * pw0[1] + R[3 * i + 2] * pw0[2]);
  double sum2 = 0.0;   // reprojection_error (:520-536)
  for (int i = 0; i < m; i++) {
    const orbfe_pnp_point& p = pts[sel[i]];
    const double x = p.Xw[0], y = p.Xw[1], z = p.Xw[2];
    const double Xc = (R[0] * x + R[1] * y + R[2] * z) + t[0];
    const double Yc = (R[3] * x + R[4] * y + R[5] * z) + t[1];
    const double inv_Zc = 1.0 / ((R[6] * x + R[7] * y + R[8] * z) + t[2]);
    const double ue = K.uc + K.fu * Xc * inv_Zc, ve = K.vc + K.fv * Yc * inv_Zc;
    const double u = p.u, v = p.v;
    sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
  }
  T.err = sum2 / m;
#pragma unroll
  for (int e = 0; e < 9; e++) T.R[e] = R[e];
#pragma unroll
  for (int e = 0; e < 3; e++) T.t[e] = t[e];
}

// compute_pose (:451-500) on the m correspondences pts[sel[0 .. m)], by all nl lanes.  Returns the winning start (0, 1, 2); its
// pose is w->st[winner].R / .t.  The caller separates the call from its next write of the PnpWork by PNP_SYNC().
PNP_HD int pnp_compute_pose(PnpWork* w, const PnpCamera& K, const orbfe_pnp_point* pts, const int32_t* sel, int m, int lane, int nl) {
  if (lane == 0) pnp_control_points(w, pts, sel, m);
  PNP_SYNC();
  for (int e = lane; e < 144; e += nl) w->A[e] = pnp_mtm_entry(w, K, pts, sel, m, e / 12, e % 12);
  PNP_SYNC();
  pnp_jacobi12(w, lane, nl);
  PNP_SYNC();
  if (lane == 0) {   // the five eigenvalues of smallest magnitude, smallest first (rows 11, 10, 9, 8, 7 of Ut), the first of equals
    for (int i = 0; i < 12; i++) w->ord[i] = i;
    for (int i = 0; i < 5; i++) {
      int best = i;
      for (int j = i + 1; j < 12; j++)
        if (fabs(w->A[13 * w->ord[j]]) < fabs(w->A[13 * w->ord[best]])) best = j;
      const int x = w->ord[i]; w->ord[i] = w->ord[best]; w->ord[best] = x;
      w->eig[i] = w->A[13 * w->ord[i]];
    }
  }
  PNP_SYNC();
  for (int e = lane; e < 48; e += nl) w->Vs[e] = w->V[(e % 12) * 12 + w->ord[e / 12]];
  PNP_SYNC();
  for (int i = lane; i < 6; i += nl) {   // compute_L_6x10 and compute_rho (:724-772): row i is the pair (a, b) of control points
    const int a = i < 3 ? 0 : i < 5 ? 1 : 2, b = i < 3 ? i + 1 : i < 5 ? i - 1 : 3;
    double dv[4][3];
#pragma unroll
    for (int v = 0; v < 4; v++)
#pragma unroll
      for (int c = 0; c < 3; c++) dv[v][c] = w->Vs[12 * v + 3 * a + c] - w->Vs[12 * v + 3 * b + c];
#define PNP_DOT(x, y) (dv[x][0] * dv[y][0] + dv[x][1] * dv[y][1] + dv[x][2] * dv[y][2])
    double* row = w->L + 10 * i;
    row[0] = PNP_DOT(0, 0); row[1] = 2.0 * PNP_DOT(0, 1); row[2] = PNP_DOT(1, 1); row[3] = 2.0 * PNP_DOT(0, 2); row[4] = 2.0 * PNP_DOT(1, 2);
    row[5] = PNP_DOT(2, 2); row[6] = 2.0 * PNP_DOT(0, 3); row[7] = 2.0 * PNP_DOT(1, 3); row[8] = 2.0 * PNP_DOT(2, 3); row[9] = PNP_DOT(3, 3);
#undef PNP_DOT
    const double d0 = w->cws[3 * a] - w->cws[3 * b], d1 = w->cws[3 * a + 1] - w->cws[3 * b + 1], d2 = w->cws[3 * a + 2] - w->cws[3 * b + 2];
    w->rho[i] = d0 * d0 + d1 * d1 + d2 * d2;
  }
  PNP_SYNC();
  for (int s = lane; s < 3; s += nl) pnp_start(w, K, pts, sel, m, s);
  PNP_SYNC();
  int N = 0;   // :491-495
  if (w->st[1].err < w->st[0].err) N = 1;
  if (w->st[2].err < w->st[N].err) N = 2;
  return N;
}

// the conventions and derived values of the solve that w holds, for lane 0 to store
PNP_HD void pnp_fill_diag(const PnpWork* w, orbfe_pnp_diag* d) {
  for (int e = 0; e < 12; e++) d->cws[e] = w->cws[e];
  for (int e = 0; e < 48; e++) d->V[e] = w->Vs[e];
  for (int e = 0; e < 5; e++) d->eig[e] = w->eig[e];
  for (int s = 0; s < 3; s++) {
    for (int e = 0; e < 4; e++) d->betas[4 * s + e] = w->st[s].betas[e];
    d->rep_errors[s] = w->st[s].err;
  }
}

// ---- launchers (pnp_kernels.hip)
#define PNP_WAVES 4   // hypotheses (waves) per workgroup of pnp_hypotheses_kernel
struct PnpLaunch {
  const orbfe_pnp_camera* camera;                                 // [P]
  const orbfe_pnp_point* points; const int32_t* n; int cap;       // [P][cap], [P]
  const int32_t* sets; const int32_t* H; int h_cap;               // [P][h_cap][4], [P]
  const int32_t* min_inliers;                                     // [P]
  orbfe_pnp_hypothesis* hyps; uint64_t* words;                    // [P][h_cap], [P][h_cap][W], W = ceil(cap / 64)
  orbfe_pnp_refine* refines; uint64_t* refine_words;              // the same shapes, rows of the prefix maxima only
  orbfe_pnp_diag* diag; orbfe_pnp_diag* refine_diag;              // [P][h_cap] or null
  orbfe_pnp_result* result; uint64_t* mask;                       // [P], [P][W]
};
void orbfe_launch_pnp_hypotheses(const PnpLaunch& L, int P, hipStream_t s);
void orbfe_launch_pnp_refine(const PnpLaunch& L, int P, hipStream_t s);
void orbfe_launch_pnp_select(const PnpLaunch& L, int P, hipStream_t s);
