// host_arith.cpp -- every user of csrc/jacobi_internal.h and pose_rotation compiled for the HOST, one plain C function per role, so
// that tests/test_jacobi_cpu.py can pin their bytes (tests/golden/jacobi_pins.npz) and compare them with LAPACK on a machine without
// a GPU.  Same flags as the library (-ffp-contract=off).  Each function runs `count` independent problems laid end to end.
#include <string.h>

#include "../../refactored_orb_slam2_amd/csrc/initializer_internal.h"
#include "../../refactored_orb_slam2_amd/csrc/pnp_internal.h"
#include "../../refactored_orb_slam2_amd/csrc/pose_internal.h"
#include "../../refactored_orb_slam2_amd/csrc/sim3_internal.h"

// the null vector of a float 4x4 (row-major): A[count][16] -> v[count][4]
extern "C" void jacobi_host_null4(const float* A, int count, float* v) {
  for (int i = 0; i < count; i++) tri_null_vector(A + 16 * i, v + 4 * i);
}

// A = U diag(w) Vt of a float 3x3: A[count][9] -> U[count][9], w[count][3], Vt[count][9]
extern "C" void jacobi_host_svd3(const float* A, int count, float* U, float* w, float* Vt) {
  for (int i = 0; i < count; i++) ini_svd3(A + 9 * i, U + 9 * i, w + 3 * i, Vt + 9 * i);
}

// the nine-column null vector: the 16 rows of A as doubles, A[count][16][9] -> v[count][9]; the nine rows of V = I are added here
extern "C" void jacobi_host_null9(const double* A, int count, float* v) {
  for (int i = 0; i < count; i++) {
    IniRow rows[25];
    static_assert(sizeof(IniRow) == 9 * sizeof(double), "one row is nine doubles");
    memcpy(rows, A + 144 * i, 16 * sizeof(IniRow));
    for (int k = 0; k < 9; k++) rows[16 + k] = ini_row_v(k);
    ini_null9_host(rows, v + 9 * i);
  }
}

// the top eigenvector of a symmetric float 4x4 from its upper triangle n00 n01 n02 n03 n11 n12 n13 n22 n23 n33: N[count][10] -> q[count][4]
extern "C" void jacobi_host_eig4(const float* N, int count, float* q) {
  for (int i = 0; i < count; i++) {
    const float* n = N + 10 * i;
    sim3_top_eigenvector(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8], n[9], q + 4 * i);
  }
}

// the in-memory two-sided form on a symmetric n x n, in place: A[count][n * n] becomes (nearly) diagonal, V[count][n * n] the eigenvectors
extern "C" void jacobi_host_twosided(double* A, double* V, int n, int count) {
  for (int i = 0; i < count; i++) jacobi_twosided_mem(A + n * n * i, V + n * n * i, n, PNP_EPS, JACOBI_SWEEPS);
}

// the in-memory one-sided form on an m x k block, in place: W[count][m * k] gets orthogonal columns, V[count][k * k] the rotations
extern "C" void jacobi_host_onesided(double* W, double* V, int m, int k, int count) {
  for (int i = 0; i < count; i++) jacobi_onesided_mem(W + m * k * i, V + k * k * i, m, k, PNP_EPS, JACOBI_SWEEPS);
}

static PoseSE3 load_pose(const double* p) {
  PoseSE3 q;
  q.qx = p[0]; q.qy = p[1]; q.qz = p[2]; q.qw = p[3]; q.tx = p[4]; q.ty = p[5]; q.tz = p[6];
  return q;
}

// p[count][7] = qx qy qz qw tx ty tz -> R[count][9]
extern "C" void jacobi_host_pose_rotation(const double* p, int count, double* R) {
  for (int i = 0; i < count; i++) pose_rotation(load_pose(p + 7 * i), R + 9 * i);
}

// p[count][7] -> T[count][12]
extern "C" void jacobi_host_pose_to_Tcw(const double* p, int count, float* T) {
  for (int i = 0; i < count; i++) pose_to_Tcw(load_pose(p + 7 * i), T + 12 * i);
}
