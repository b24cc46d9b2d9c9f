// gba_kernels.hip -- Optimizer::BundleAdjustment (L/src/Optimizer.cc:43-231) of ONE map of up to ORBFE_GBA_MAX_KEYFRAMES keyframes
// across the whole device: the schedule of ba_kernels.hip (one optimize(n), robust or not, no classification) under a second
// choreography.  lba_optimize.h spreads the items of a g2o BlockSolver_6_3 trial over one workgroup with barriers between the
// phases; here every phase is a launch over the grid and the launch boundary is the only grid-wide synchronisation: no grid
// barrier, no cooperative launch, no flag anybody spins on, and every device loop is bounded by a count known at its launch.
//
// The arithmetic is lba_internal.h's, one item per call, over an LbaWs carved from the workspace whose pose arrays and row-block
// maps live in HBM.  Every sum keeps the owner and the order lba_optimize.h gives it, so a problem that fits both forms gives the
// same bytes in both:
//   plan       once per call (BundleAdjustment never changes an edge's level): the edge range per point; the edge list per free
//              keyframe by a counting sort over chunks of GBA_CHUNK edges, which keeps edge order; the row-block maps; which pairs
//              of row blocks share a point
//   build      a lane per point (lba_point_build), a lane per (row block, entry of Hpp | bp) (lba_kf_sum)
//   trial      lba_point_dinv per point; lba_bschur per row; lba_schur_entry per entry of a pair that shares a point, zeros
//              elsewhere; the blocked L L^T; the two triangular solves; lba_point_update / lba_pose_update; lba_point_chi
//   control    ONE workgroup of LBA_THREADS sums the shares the grid left in HBM -- lane tid the points tid, tid + 256, ... edge by
//              edge and term by term as lba_optimize.h's lane would have, then row blocks tid, tid + 256, ... -- runs lm_reduce.h's
//              reduction unchanged and the Levenberg bookkeeping of lm_internal.h, and leaves a control record for the host loop
// L L^T: right-looking over tiles of GBA_TB rows.  Per tile column: the diagonal tile is factored by one workgroup, a column at a
// time as lba_optimize.h does; every tile below it is solved against it by a workgroup, a column at a time; every trailing tile is
// updated by a workgroup.  An entry (i, j) therefore sees S[i][j] -= L[i][k] * L[j][k] for k ascending, each product subtracted on
// its own (-ffp-contract=off), then the division by L[j][j]: the operations and the order of lba_cholesky_solve.  That rules out
// v_mfma_f64_16x16x4_f64, which fuses and sums four k at a time in an order of its own.
// The triangular solves are blocked over the same tiles, a launch per tile column: b[i] -= S[i][k] * y[k] for k ascending and the
// mirror for the back solve, the per-entry order of lba_optimize.h.
// A pivot that is not > 0 sets dev->fail; every later launch of the trial returns at once on it.
#include "gba_internal.h"
#include "lba_optimize.h"

#define GBA_THREADS 256

struct GbaArgs {
  GbaLaunch L;
  GbaWs G;
  int robust;
};

__device__ __forceinline__ LbaWs gba_ws(const GbaArgs& A) {
  LbaWs W = A.G.W;
  W.K = A.G.dev->K;
  return W;
}
__device__ __forceinline__ size_t gba_gid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

// ---- plan -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GBA_THREADS) void gba_begin(GbaArgs A) {   // one workgroup
  GbaDev& D = *A.G.dev;
  if (threadIdx.x != 0) return;
  D.K.fx = (double)A.L.camera->fx;
  D.K.fy = (double)A.L.camera->fy;
  D.K.cx = (double)A.L.camera->cx;
  D.K.cy = (double)A.L.camera->cy;
  D.K.bf = (double)A.L.camera->mbf;
  int nf = 0;
  for (int k = 0; k < A.L.n_kf; k++) {
    if (!A.L.fixed[k]) {
      A.G.W.kf_of_fi[nf] = k;
      A.G.fi_of_kf[k] = nf++;
    } else {
      A.G.fi_of_kf[k] = -1;
    }
  }
  D.n_free = nf;
  D.invalid = 0;
  D.fail = 0;
  D.ns = 0;
  D.it = D.qmax = D.iterations = D.trials = 0;
  D.lambda = 0.0;
  D.ni = 2.0;
  D.current_chi = D.chi2_first = D.rho = 0.0;
}

__global__ __launch_bounds__(GBA_THREADS) void gba_validate(GbaArgs A) {
  const size_t i = gba_gid();
  if (i >= (size_t)A.L.n_edges) return;
  if (!lba_edge_valid(A.L.edges, (int)i, A.L.n_kf, A.L.n_points)) A.G.dev->invalid = 1;
}

__global__ __launch_bounds__(GBA_THREADS) void gba_decide(GbaArgs A) {   // one workgroup
  if (threadIdx.x != 0) return;
  GbaDev& D = *A.G.dev;
  D.state = D.invalid ? LBA_REFUSED : (D.n_free == 0 || A.L.n_edges == 0) ? LBA_IDLE : LBA_READY;
  GbaControl& C = *A.G.control;
  C.action = D.state == LBA_READY ? GBA_BUILD : GBA_DONE;
  C.pop = 0;
  C.state = D.state;
  C.n_free = D.n_free;
  C.ns = 0;
  C.iterations = C.trials = C.reserved = 0;
  C.lambda = C.chi2_first = C.chi2 = 0.0;
}

// The inputs of a problem that is refused or has nothing to do go through as they are
__global__ __launch_bounds__(GBA_THREADS) void gba_pass(GbaArgs A) {
  if (A.G.dev->state == LBA_READY) return;
  const size_t j = gba_gid();
  if (j < (size_t)A.L.n_kf * 12) A.L.poses_out[j] = A.L.poses[j];
  if (j < (size_t)A.L.n_points * 3)
    A.L.points_out[j] = reinterpret_cast<const float*>(A.L.points + (j / 3) * (size_t)A.L.point_stride)[j % 3];
  if (j == 0) {
    orbfe_ba_result res;
    res.rounds = A.G.dev->state == LBA_IDLE ? 0 : -1;
    res.n_free = A.G.dev->n_free;
    res.n_edges = A.L.n_edges;
    res.iterations = res.trials = res.reserved = 0;
    res.chi2_first = res.chi2_final = 0.0;
    *A.L.result = res;
  }
}

__global__ __launch_bounds__(GBA_THREADS) void gba_widen(GbaArgs A) {
  if (A.G.dev->state != LBA_READY) return;
  const LbaWs& W = A.G.W;
  const size_t j = gba_gid();
  if (j < (size_t)A.L.n_kf) {
    W.pose[j] = pose_from_Tcw(A.L.poses + j * 12);
    W.slot_of_kf[j] = -1;
  }
  if (j < (size_t)A.L.n_points) {
    const float* X = reinterpret_cast<const float*>(A.L.points + j * (size_t)A.L.point_stride);
    W.pt[3 * j] = (double)X[0];
    W.pt[3 * j + 1] = (double)X[1];
    W.pt[3 * j + 2] = (double)X[2];
    W.pt_start[j] = 0;
    W.pt_end[j] = 0;
    W.pt_active[j] = 0;
  }
  const size_t F = (size_t)A.L.n_kf;
  for (size_t t = j; t < F * F; t += (size_t)gridDim.x * blockDim.x) A.G.pairs[t] = 0;
}

__global__ __launch_bounds__(GBA_THREADS) void gba_edge_ranges(GbaArgs A) {
  if (A.G.dev->state != LBA_READY) return;
  const LbaWs& W = A.G.W;
  const size_t g = gba_gid();
  if (g >= (size_t)A.L.n_edges) return;
  const int i = (int)g, p = W.edges[i].point;
  if (i == 0 || W.edges[i - 1].point != p) W.pt_start[p] = i;
  if (i == W.n_e - 1 || W.edges[i + 1].point != p) W.pt_end[p] = i + 1;
  W.level[i] = 0;
  W.chi2[i] = 0.0;
}

// A workgroup per chunk of GBA_CHUNK edges: the edges of every free keyframe in the chunk (integer counts in HBM, one owner each)
__global__ __launch_bounds__(GBA_THREADS) void gba_chunk_count(GbaArgs A) {
  if (A.G.dev->state != LBA_READY) return;
  const int F = A.L.n_kf, c = blockIdx.x;
  int* cnt = A.G.chunk_cnt + (size_t)c * F;
  const int e0 = c * GBA_CHUNK, e1 = min(A.L.n_edges, e0 + GBA_CHUNK);
  const int nf = A.G.dev->n_free;
  // lane t owns the free keyframes t, t + 256, ...: it walks the chunk once per keyframe it owns -- no atomics
  for (int fi = threadIdx.x; fi < nf; fi += GBA_THREADS) cnt[fi] = 0;
  __syncthreads();
  __shared__ int sfi[GBA_THREADS];
  for (int base = e0; base < e1; base += GBA_THREADS) {
    const int i = base + threadIdx.x;
    sfi[threadIdx.x] = i < e1 ? A.G.fi_of_kf[A.L.edges[i].kf] : -1;
    __syncthreads();
    const int m = min(GBA_THREADS, e1 - base);
    for (int fi = threadIdx.x; fi < nf; fi += GBA_THREADS) {
      int n = 0;
      for (int t = 0; t < m; t++) n += sfi[t] == fi ? 1 : 0;
      cnt[fi] += n;
    }
    __syncthreads();
  }
}

// A lane per free keyframe: its total, and every chunk's count turned into the offset of that chunk inside the keyframe's list
__global__ __launch_bounds__(GBA_THREADS) void gba_chunk_offsets(GbaArgs A, int chunks) {
  if (A.G.dev->state != LBA_READY) return;
  const size_t fi = gba_gid();
  if (fi >= (size_t)A.G.dev->n_free) return;
  const int F = A.L.n_kf;
  int o = 0;
  for (int c = 0; c < chunks; c++) {
    int* q = A.G.chunk_cnt + (size_t)c * F + fi;
    const int n = *q;
    *q = o;
    o += n;
  }
  A.G.W.fi_of_slot[fi] = o;   // the total, until gba_slots has read it
}

// initializeOptimization(0): the lists' ranges, and a row block for every free keyframe with an edge (every edge is at level 0)
__global__ __launch_bounds__(GBA_THREADS) void gba_slots(GbaArgs A) {   // one workgroup
  GbaDev& D = *A.G.dev;
  if (D.state != LBA_READY || threadIdx.x != 0) return;
  const LbaWs& W = A.G.W;
  int o = 0, ns = 0;
  for (int fi = 0; fi < D.n_free; fi++) {
    const int n = W.fi_of_slot[fi], kf = W.kf_of_fi[fi];
    W.kf_start[fi] = o;
    o += n;
    if (n > 0) {
      W.fi_of_slot[ns] = fi;   // ns <= fi: the totals still to be read are not overwritten
      W.slot_of_kf[kf] = ns++;
    }
  }
  W.kf_start[D.n_free] = o;
  D.ns = ns;
  A.G.control->ns = ns;
}

// A workgroup per chunk: every edge to its place in its keyframe's list, in edge order
__global__ __launch_bounds__(GBA_THREADS) void gba_chunk_fill(GbaArgs A) {
  if (A.G.dev->state != LBA_READY) return;
  const LbaWs& W = A.G.W;
  const int F = A.L.n_kf, c = blockIdx.x, tid = threadIdx.x;
  int* off = A.G.chunk_cnt + (size_t)c * F;   // running offset of this chunk inside every keyframe's list
  const int e0 = c * GBA_CHUNK, e1 = min(A.L.n_edges, e0 + GBA_CHUNK);
  const int nf = A.G.dev->n_free;
  __shared__ int sfi[GBA_THREADS];
  for (int base = e0; base < e1; base += GBA_THREADS) {
    const int i = base + tid;
    const int fi = i < e1 ? A.G.fi_of_kf[A.L.edges[i].kf] : -1;
    sfi[tid] = fi;
    __syncthreads();
    if (fi >= 0) {
      int rank = 0;
      for (int t = 0; t < tid; t++) rank += sfi[t] == fi ? 1 : 0;
      W.kf_list[W.kf_start[fi] + off[fi] + rank] = i;
    }
    __syncthreads();
    const int m = min(GBA_THREADS, e1 - base);
    for (int f = tid; f < nf; f += GBA_THREADS) {
      int n = 0;
      for (int t = 0; t < m; t++) n += sfi[t] == f ? 1 : 0;
      off[f] += n;
    }
    __syncthreads();
  }
}

// A lane per point: every pair of its row blocks shares it (the edges of a point ascend in their keyframes, so in their row blocks)
__global__ __launch_bounds__(GBA_THREADS) void gba_pairs(GbaArgs A) {
  if (A.G.dev->state != LBA_READY) return;
  const LbaWs& W = A.G.W;
  const size_t p = gba_gid();
  if (p >= (size_t)A.L.n_points) return;
  const size_t F = (size_t)A.L.n_kf;
  for (int a = W.pt_start[p]; a < W.pt_end[p]; a++) {
    const int sa = W.slot_of_kf[W.edges[a].kf];
    if (sa < 0) continue;
    for (int b = a + 1; b < W.pt_end[p]; b++) {
      const int sb = W.slot_of_kf[W.edges[b].kf];
      if (sb >= 0) A.G.pairs[(size_t)sa * F + sb] = 1;
    }
  }
}

// ---- build --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GBA_THREADS) void gba_build_points(GbaArgs A, double delta_mono) {
  const size_t p = gba_gid();
  if (p >= (size_t)A.L.n_points) return;
  const LbaWs W = gba_ws(A);
  double chi = 0.0, maxd = 0.0;   // the control kernel sums the edges' and the points' shares
  lba_point_build(W, (int)p, A.robust != 0, &chi, &maxd, delta_mono);
}

__global__ __launch_bounds__(GBA_THREADS) void gba_build_kf(GbaArgs A) {
  const size_t t = gba_gid();
  if (t >= (size_t)A.G.dev->ns * LBA_EKF) return;
  const LbaWs& W = A.G.W;
  lba_kf_sum(W, W.fi_of_slot[t / LBA_EKF], (int)(t % LBA_EKF));
}

// ---- trial --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GBA_THREADS) void gba_dinv(GbaArgs A) {
  const size_t p = gba_gid();
  if (p >= (size_t)A.L.n_points) return;
  lba_point_dinv(A.G.W, (int)p, A.G.dev->lambda);
}

__global__ __launch_bounds__(GBA_THREADS) void gba_bschur(GbaArgs A) {
  const size_t t = gba_gid();
  if (t >= (size_t)A.G.dev->ns * 6) return;
  A.G.b[t] = lba_bschur(A.G.W, A.G.W.fi_of_slot[t / 6], (int)(t % 6));
}

// blockIdx.y: row block j; a lane per entry (i, r, c) of blocks i <= j
__global__ __launch_bounds__(GBA_THREADS) void gba_schur(GbaArgs A) {
  const LbaWs& W = A.G.W;
  const int ns = A.G.dev->ns, j = blockIdx.y;
  const size_t t = gba_gid();
  if (j >= ns || t >= (size_t)(j + 1) * 36) return;
  const int i = (int)(t / 36), r = (int)(t % 36) / 6, c = (int)(t % 6);
  if (i == j && r > c) return;
  const size_t n = (size_t)6 * ns;
  double s = 0.0;
  if (i == j || A.G.pairs[(size_t)i * A.L.n_kf + j]) s = lba_schur_entry(W, W.fi_of_slot[i], W.fi_of_slot[j], r, c, A.G.dev->lambda);
  W.S[(size_t)(6 * j + c) * n + (6 * i + r)] = s;
}

// Tile (K, K): L L^T a column at a time in LDS; S keeps its diagonal, L's goes to diag
__global__ __launch_bounds__(GBA_THREADS) void gba_chol_diag(double* S, double* diag, GbaDev* dev, int K) {
  GbaDev& D = *dev;
  if (D.fail) return;
  __shared__ double T[GBA_TB][GBA_TB + 1];
  const int tid = threadIdx.x, n = 6 * D.ns, r0 = K * GBA_TB, m = min(GBA_TB, n - r0);
  for (int t = tid; t < m * m; t += GBA_THREADS) {
    const int i = t / m, j = t % m;
    if (j <= i) T[i][j] = S[(size_t)(r0 + i) * n + r0 + j];
  }
  __syncthreads();
  for (int k = 0; k < m; k++) {
    const double d = T[k][k];
    if (!(d > 0.0)) {   // uniform: every lane read the same value
      if (tid == 0) D.fail = 1;
      return;
    }
    const double lkk = sqrt(d);
    if (tid == 0) diag[r0 + k] = lkk;
    for (int i = k + 1 + tid; i < m; i += GBA_THREADS) T[i][k] = T[i][k] / lkk;
    __syncthreads();
    for (int i = k + 1 + (tid >> 4); i < m; i += GBA_THREADS / 16) {
      const double lik = T[i][k];
      for (int j = k + 1 + (tid & 15); j <= i; j += 16) T[i][j] -= lik * T[j][k];
    }
    __syncthreads();
  }
  for (int t = tid; t < m * m; t += GBA_THREADS) {
    const int i = t / m, j = t % m;
    if (j < i) S[(size_t)(r0 + i) * n + r0 + j] = T[i][j];
  }
}

// Tile (K + 1 + blockIdx.x, K): its rows against the factored diagonal tile, a column at a time
__global__ __launch_bounds__(GBA_THREADS) void gba_chol_panel(double* S, const double* diag, const GbaDev* dev, int K) {
  const GbaDev& D = *dev;
  if (D.fail) return;
  __shared__ double T[GBA_TB][GBA_TB + 1], Ld[GBA_TB][GBA_TB + 1];
  const int tid = threadIdx.x, n = 6 * D.ns, c0 = K * GBA_TB, r0 = (K + 1 + blockIdx.x) * GBA_TB, m = min(GBA_TB, n - r0);
  for (int t = tid; t < GBA_TB * GBA_TB; t += GBA_THREADS) {
    const int i = t / GBA_TB, j = t % GBA_TB;
    if (i < m) T[i][j] = S[(size_t)(r0 + i) * n + c0 + j];
    if (j < i) Ld[i][j] = S[(size_t)(c0 + i) * n + c0 + j];
  }
  __syncthreads();
  for (int k = 0; k < GBA_TB; k++) {
    const double lkk = diag[c0 + k];
    for (int i = tid; i < m; i += GBA_THREADS) T[i][k] = T[i][k] / lkk;
    __syncthreads();
    for (int i = tid >> 4; i < m; i += GBA_THREADS / 16) {
      const double lik = T[i][k];
      for (int j = k + 1 + (tid & 15); j < GBA_TB; j += 16) T[i][j] -= lik * Ld[j][k];
    }
    __syncthreads();
  }
  for (int t = tid; t < m * GBA_TB; t += GBA_THREADS) S[(size_t)(r0 + t / GBA_TB) * n + c0 + t % GBA_TB] = T[t / GBA_TB][t % GBA_TB];
}

// Tile (I, J), K < J <= I, I = K + 1 + blockIdx.y, J = K + 1 + blockIdx.x: minus L[I][K] L[J][K]^T, one k at a time
__global__ __launch_bounds__(GBA_THREADS) void gba_chol_update(double* S, const GbaDev* dev, int K) {
  const GbaDev& D = *dev;
  if (D.fail || blockIdx.x > blockIdx.y) return;
  __shared__ double La[GBA_TB][GBA_TB + 1], Lb[GBA_TB][GBA_TB + 1];
  const int tid = threadIdx.x, n = 6 * D.ns, c0 = K * GBA_TB;
  const int r0 = (K + 1 + blockIdx.y) * GBA_TB, q0 = (K + 1 + blockIdx.x) * GBA_TB, m = min(GBA_TB, n - r0);
  for (int t = tid; t < GBA_TB * GBA_TB; t += GBA_THREADS) {
    const int i = t / GBA_TB, k = t % GBA_TB;
    if (i < m) La[i][k] = S[(size_t)(r0 + i) * n + c0 + k];
    Lb[i][k] = q0 + i < n ? S[(size_t)(q0 + i) * n + c0 + k] : 0.0;
  }
  __syncthreads();
  const bool diagonal = blockIdx.x == blockIdx.y;
  constexpr int E = GBA_TB / 16;   // a lane's micro-tile: rows ti + 16 a, columns tj + 16 b
  const int ti = tid >> 4, tj = tid & 15;
  double acc[E][E];
#pragma unroll
  for (int a = 0; a < E; a++)
#pragma unroll
    for (int b = 0; b < E; b++) {
      const int i = ti + 16 * a, j = tj + 16 * b;
      acc[a][b] = (i < m && (!diagonal || j <= i)) ? S[(size_t)(r0 + i) * n + q0 + j] : 0.0;
    }
#pragma unroll 4
  for (int k = 0; k < GBA_TB; k++) {
    double la[E], lb[E];
#pragma unroll
    for (int a = 0; a < E; a++) la[a] = La[ti + 16 * a][k];
#pragma unroll
    for (int b = 0; b < E; b++) lb[b] = Lb[tj + 16 * b][k];
#pragma unroll
    for (int a = 0; a < E; a++)
#pragma unroll
      for (int b = 0; b < E; b++) acc[a][b] -= la[a] * lb[b];
  }
#pragma unroll
  for (int a = 0; a < E; a++)
#pragma unroll
    for (int b = 0; b < E; b++) {
      const int i = ti + 16 * a, j = tj + 16 * b;
      if (i < m && (!diagonal || j <= i)) S[(size_t)(r0 + i) * n + q0 + j] = acc[a][b];
    }
}

// L y = b, a launch per tile column K: every workgroup solves the tile's rows in LDS (the same bits in each), a column at a time as
// lba_optimize.h does, then takes 256 of the rows below the tile through the tile's columns, k ascending: b[i] -= S[i][k] * y[k]
__global__ __launch_bounds__(GBA_THREADS) void gba_solve_forward(const double* S, const double* diag, double* b, double* y, const GbaDev* dev,
                                                                 int K) {
  if (dev->fail) return;
  __shared__ double Ld[GBA_TB][GBA_TB + 1], yb[GBA_TB];
  const int tid = threadIdx.x, n = 6 * dev->ns, c0 = K * GBA_TB, m = min(GBA_TB, n - c0);
  for (int t = tid; t < m * m; t += GBA_THREADS) {
    const int i = t / m, j = t % m;
    if (j < i) Ld[i][j] = S[(size_t)(c0 + i) * n + c0 + j];
  }
  if (tid < m) yb[tid] = b[c0 + tid];
  __syncthreads();
  for (int k = 0; k < m; k++) {
    if (tid == 0) yb[k] = yb[k] / diag[c0 + k];
    __syncthreads();
    if (tid > k && tid < m) yb[tid] -= Ld[tid][k] * yb[k];
    __syncthreads();
  }
  if (blockIdx.x == 0 && tid < m) y[c0 + tid] = yb[tid];
  const size_t i = (size_t)c0 + m + (size_t)blockIdx.x * GBA_THREADS + tid;
  if (i >= (size_t)n) return;
  const double* row = S + i * n + c0;
  double acc = b[i];
  for (int k = 0; k < m; k++) acc -= row[k] * yb[k];
  b[i] = acc;
}

// L^T x = y, a launch per tile column K from the last one up: the tile's rows in LDS, k descending, then 256 of the rows above the
// tile through the tile's rows, k descending: y[i] -= S[k][i] * x[k]
__global__ __launch_bounds__(GBA_THREADS) void gba_solve_backward(const double* S, const double* diag, double* y, double* x, const GbaDev* dev,
                                                                  int K) {
  if (dev->fail) return;
  __shared__ double Ld[GBA_TB][GBA_TB + 1], xb[GBA_TB];
  const int tid = threadIdx.x, n = 6 * dev->ns, c0 = K * GBA_TB, m = min(GBA_TB, n - c0);
  for (int t = tid; t < m * m; t += GBA_THREADS) {
    const int i = t / m, j = t % m;
    if (j < i) Ld[i][j] = S[(size_t)(c0 + i) * n + c0 + j];
  }
  if (tid < m) xb[tid] = y[c0 + tid];
  __syncthreads();
  for (int k = m - 1; k >= 0; k--) {
    if (tid == 0) xb[k] = xb[k] / diag[c0 + k];
    __syncthreads();
    if (tid < k) xb[tid] -= Ld[k][tid] * xb[k];
    __syncthreads();
  }
  if (blockIdx.x == 0 && tid < m) x[c0 + tid] = xb[tid];
  const size_t i = (size_t)blockIdx.x * GBA_THREADS + tid;
  if (i >= (size_t)c0) return;
  double acc = y[i];
  for (int k = m - 1; k >= 0; k--) acc -= S[(size_t)(c0 + k) * n + i] * xb[k];
  y[i] = acc;
}

__global__ __launch_bounds__(GBA_THREADS) void gba_update(GbaArgs A) {
  const GbaDev& D = *A.G.dev;
  if (D.fail) return;
  const size_t g = gba_gid();
  double scale = 0.0;   // the control kernel sums the terms
  if (g < (size_t)A.L.n_points) lba_point_update(A.G.W, (int)g, D.lambda, A.G.x, &scale);
  if (g < (size_t)D.ns) lba_pose_update(A.G.W, (int)g, D.lambda, A.G.x, &scale);
}

__global__ __launch_bounds__(GBA_THREADS) void gba_chi(GbaArgs A, double delta_mono) {
  if (A.G.dev->fail) return;
  const size_t p = gba_gid();
  if (p >= (size_t)A.L.n_points) return;
  const LbaWs W = gba_ws(A);
  double chi = 0.0;
  lba_point_chi(W, (int)p, A.robust != 0, &chi, delta_mono);
}

__global__ __launch_bounds__(GBA_THREADS) void gba_pop(GbaArgs A) {
  const LbaWs& W = A.G.W;
  const size_t g = gba_gid();
  if (g < (size_t)A.L.n_points) lba_point_pop(W, (int)g);
  if (g < (size_t)A.G.dev->ns) {
    const int kf = W.kf_of_fi[W.fi_of_slot[g]];
    W.pose[kf] = W.pose_bak[kf];
  }
}

// ---- control: ONE workgroup of LBA_THREADS ----------------------------------------------------------------------------------------
// after_trial == 0: behind a build -- the build's chi2, and lambda from the largest diagonal entry in iteration 0.
// after_trial == 1: behind a trial -- its chi2 and computeScale, lm_trial_scaled, and the loop rules of lba_optimize_call.
__global__ __launch_bounds__(LBA_THREADS) void gba_control(GbaArgs A, double delta_mono, int after_trial) {
  __shared__ double red[LBA_WAVES * 2], tot[2], red_m[LBA_WAVES];
  const int tid = threadIdx.x;
  const LbaWs W = gba_ws(A);
  GbaDev& D = *A.G.dev;
  GbaControl& C = *A.G.control;
  const bool robust = A.robust != 0, ok2 = !D.fail;
  const int ns = D.ns;
  const double lambda = D.lambda;
  double u[2] = {0.0, 0.0};
  if (!after_trial || ok2) {
    if (after_trial) {
      for (int p = tid; p < W.n_pt; p += LBA_THREADS)
        if (W.pt_active[p]) gba_scale3(W, p, lambda, &u[1]);
      for (int s = tid; s < ns; s += LBA_THREADS) gba_scale6(W, s, lambda, A.G.x, &u[1]);
    }
    for (int p = tid; p < W.n_pt; p += LBA_THREADS)
      for (int i = W.pt_start[p]; i < W.pt_end[p]; i++) u[0] += gba_edge_rho(W, i, robust, delta_mono);
    lm_reduce<2, 2, LBA_WAVES>(u, red, tot, tid);
  }
  if (!after_trial) {
    double lam = D.lambda, ni = D.ni;
    if (D.it == 0) {   // computeLambdaInit over every active vertex
      double maxd = 0.0;
      for (int p = tid; p < W.n_pt; p += LBA_THREADS)
        if (W.pt_active[p]) {
          maxd = fmax(fabs(W.Hll[(size_t)9 * p]), maxd);
          maxd = fmax(fabs(W.Hll[(size_t)9 * p + 4]), maxd);
          maxd = fmax(fabs(W.Hll[(size_t)9 * p + 8]), maxd);
        }
      for (int t = tid; t < ns * 21; t += LBA_THREADS)
        if (lba_is_diag(t % 21)) maxd = fmax(fabs(W.Hpp[21 * W.fi_of_slot[t / 21] + t % 21]), maxd);
      maxd = lm_reduce_max<LBA_WAVES>(maxd, red_m, tid);
      lam = 1e-5 * maxd;
      ni = 2.0;
    }
    const double chi = tot[0];
    __syncthreads();
    if (tid == 0) {
      D.current_chi = chi;
      if (D.it == 0) D.chi2_first = chi;
      D.lambda = lam;
      D.ni = ni;
      D.rho = 0.0;
      D.qmax = 0;
      D.fail = 0;
      C.action = GBA_TRIAL;
      C.pop = 0;
      C.lambda = lam;
      C.chi2_first = D.chi2_first;
      C.chi2 = chi;
    }
    return;
  }
  double temp_chi = 0.0, scale = 0.0;
  if (ok2) {
    temp_chi = tot[0];
    scale = tot[1];
  }
  __syncthreads();
  if (tid != 0) return;
  LmState lm;
  lm.lambda = D.lambda;
  lm.ni = D.ni;
  double rho = 0.0, current_chi = D.current_chi;
  int qmax = D.qmax, pop = 0;
  bool broke = false;
  D.trials++;
  if (lm_trial_scaled(lm, ok2, current_chi, temp_chi, scale, &rho)) {
    current_chi = temp_chi;
  } else {
    pop = ok2 ? 1 : 0;
    if (!isfinite(lm.lambda)) broke = true;
  }
  if (!broke) qmax++;
  int action = GBA_TRIAL;
  if (broke || !(rho < 0 && qmax < 10)) {
    D.iterations++;
    D.it++;
    action = (qmax == 10 || rho == 0 || !isfinite(lm.lambda) || D.it >= A.L.n_iterations) ? GBA_DONE : GBA_BUILD;
  }
  D.lambda = lm.lambda;
  D.ni = lm.ni;
  D.rho = rho;
  D.qmax = qmax;
  D.current_chi = current_chi;
  D.fail = 0;
  C.action = action;
  C.pop = pop;
  C.iterations = D.iterations;
  C.trials = D.trials;
  C.lambda = lm.lambda;
  C.chi2_first = D.chi2_first;
  C.chi2 = current_chi;
}

// ---- write-back: every keyframe through Converter::toCvMat(SE3Quat), a point without an edge as it came -----------------------------
__global__ __launch_bounds__(GBA_THREADS) void gba_write(GbaArgs A) {
  const LbaWs& W = A.G.W;
  const GbaDev& D = *A.G.dev;
  const size_t g = gba_gid();
  if (g < (size_t)A.L.n_kf) {
    float T[12];
    pose_to_Tcw(W.pose[g], T);
#pragma unroll
    for (int j = 0; j < 12; j++) A.L.poses_out[g * 12 + j] = T[j];
  }
  if (g < (size_t)A.L.n_points) {
    const float* X = reinterpret_cast<const float*>(A.L.points + g * (size_t)A.L.point_stride);
    const bool seen = W.pt_start[g] < W.pt_end[g];
#pragma unroll
    for (int j = 0; j < 3; j++) A.L.points_out[g * 3 + j] = seen ? (float)W.pt[3 * g + j] : X[j];
  }
  if (g == 0) {
    orbfe_ba_result res;
    res.rounds = 1;
    res.n_free = D.n_free;
    res.n_edges = A.L.n_edges;
    res.iterations = D.iterations;
    res.trials = D.trials;
    res.reserved = 0;
    res.chi2_first = D.chi2_first;
    res.chi2_final = D.current_chi;
    *A.L.result = res;
  }
}

// ---- the host loop ------------------------------------------------------------------------------------------------------------------
static inline dim3 grid_for(size_t items) { return dim3((unsigned)std::max<size_t>(1, (items + GBA_THREADS - 1) / GBA_THREADS)); }

namespace {
struct Phases {   // stream-event times per phase, only when somebody asks for them
  float* ms;
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  Phases(float* ms, hipStream_t s) : ms(ms), s(s) {
    if (ms && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)) this->ms = nullptr;
  }
  ~Phases() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void begin() {
    if (ms) (void)hipEventRecord(a, s);
  }
  void end(int phase) {
    if (!ms) return;
    float t = 0.f;
    (void)hipEventRecord(b, s);
    if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&t, a, b) == hipSuccess) ms[phase] += t;
  }
};
}   // namespace

hipError_t orbfe_run_gba(const GbaLaunch& L, const GbaWs& G, GbaControl* pinned, hipStream_t s, float* phase_ms) {
  GbaArgs A;
  A.L = L;
  A.G = G;
  A.G.W.n_kf = L.n_kf;
  A.G.W.n_pt = L.n_points;
  A.G.W.n_e = L.n_edges;
  A.G.W.n_free = 0;
  A.G.W.edges = L.edges;
  A.robust = (L.flags & ORBFE_BA_ROBUST) ? 1 : 0;
  const double delta_mono = ba_delta_mono();
  const int chunks = (int)gba_chunks(L.n_edges);
  const size_t items = std::max<size_t>(std::max<size_t>((size_t)L.n_kf * 12, (size_t)L.n_points * 3), 1);
  const dim3 one(1), wg(GBA_THREADS), g_pt = grid_for((size_t)L.n_points), g_e = grid_for((size_t)L.n_edges);
  Phases ph(phase_ms, s);
  hipError_t e;
  auto read_control = [&]() -> hipError_t {
    ph.begin();
    hipError_t r = hipMemcpyAsync(pinned, G.control, sizeof(GbaControl), hipMemcpyDeviceToHost, s);
    if (r == hipSuccess) r = hipStreamSynchronize(s);
    ph.end(GBA_PH_CONTROL);
    return r;
  };

  // the plan, once per call
  ph.begin();
  hipLaunchKernelGGL(gba_begin, one, wg, 0, s, A);
  hipLaunchKernelGGL(gba_validate, g_e, wg, 0, s, A);
  hipLaunchKernelGGL(gba_decide, one, wg, 0, s, A);
  hipLaunchKernelGGL(gba_pass, grid_for(items), wg, 0, s, A);
  hipLaunchKernelGGL(gba_widen, grid_for(std::max((size_t)L.n_kf, (size_t)L.n_points)), wg, 0, s, A);
  hipLaunchKernelGGL(gba_edge_ranges, g_e, wg, 0, s, A);
  if (chunks > 0) hipLaunchKernelGGL(gba_chunk_count, dim3(chunks), wg, 0, s, A);
  hipLaunchKernelGGL(gba_chunk_offsets, grid_for((size_t)L.n_kf), wg, 0, s, A, chunks);
  hipLaunchKernelGGL(gba_slots, one, wg, 0, s, A);
  if (chunks > 0) hipLaunchKernelGGL(gba_chunk_fill, dim3(chunks), wg, 0, s, A);
  hipLaunchKernelGGL(gba_pairs, g_pt, wg, 0, s, A);
  ph.end(GBA_PH_PLAN);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = read_control()) != hipSuccess) return e;
  if (pinned->state != LBA_READY) return hipSuccess;
  const int ns = pinned->ns, n = 6 * ns, tiles = (n + GBA_TB - 1) / GBA_TB;

  // at most n_iterations x 10 trials, one read of the control record each
  const int max_trials = L.n_iterations * 10;
  int action = GBA_BUILD;
  for (int trial = 0; trial < max_trials && action != GBA_DONE; trial++) {
    if (action == GBA_BUILD) {
      ph.begin();
      hipLaunchKernelGGL(gba_build_points, g_pt, wg, 0, s, A, delta_mono);
      hipLaunchKernelGGL(gba_build_kf, grid_for((size_t)ns * LBA_EKF), wg, 0, s, A);
      hipLaunchKernelGGL(gba_control, one, dim3(LBA_THREADS), 0, s, A, delta_mono, 0);
      ph.end(GBA_PH_BUILD);
    }
    ph.begin();
    hipLaunchKernelGGL(gba_dinv, g_pt, wg, 0, s, A);
    hipLaunchKernelGGL(gba_bschur, grid_for((size_t)n), wg, 0, s, A);
    hipLaunchKernelGGL(gba_schur, dim3(grid_for((size_t)ns * 36).x, std::max(ns, 1)), wg, 0, s, A);   // ns == 0: every edge on a fixed keyframe
    ph.end(GBA_PH_SCHUR);
    ph.begin();
    for (int K = 0; K < tiles; K++) {
      hipLaunchKernelGGL(gba_chol_diag, one, wg, 0, s, G.W.S, G.diag, G.dev, K);
      const int below = tiles - K - 1;
      if (below > 0) {
        hipLaunchKernelGGL(gba_chol_panel, dim3(below), wg, 0, s, G.W.S, (const double*)G.diag, (const GbaDev*)G.dev, K);
        hipLaunchKernelGGL(gba_chol_update, dim3(below, below), wg, 0, s, G.W.S, (const GbaDev*)G.dev, K);
      }
    }
    ph.end(GBA_PH_FACTOR);
    ph.begin();
    for (int K = 0; K < tiles; K++) {
      const int below = n - std::min(n, (K + 1) * GBA_TB);
      hipLaunchKernelGGL(gba_solve_forward, grid_for((size_t)below), wg, 0, s, (const double*)G.W.S, (const double*)G.diag, G.b, G.y,
                         (const GbaDev*)G.dev, K);
    }
    for (int K = tiles - 1; K >= 0; K--)
      hipLaunchKernelGGL(gba_solve_backward, grid_for((size_t)K * GBA_TB), wg, 0, s, (const double*)G.W.S, (const double*)G.diag, G.y, G.x,
                         (const GbaDev*)G.dev, K);
    ph.end(GBA_PH_SOLVE);
    ph.begin();
    hipLaunchKernelGGL(gba_update, grid_for(std::max((size_t)L.n_points, (size_t)ns)), wg, 0, s, A);
    hipLaunchKernelGGL(gba_chi, g_pt, wg, 0, s, A, delta_mono);
    hipLaunchKernelGGL(gba_control, one, dim3(LBA_THREADS), 0, s, A, delta_mono, 1);
    ph.end(GBA_PH_UPDATE);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = read_control()) != hipSuccess) return e;
    action = pinned->action;
    if (pinned->pop) hipLaunchKernelGGL(gba_pop, grid_for(std::max((size_t)L.n_points, (size_t)ns)), wg, 0, s, A);
  }
  hipLaunchKernelGGL(gba_write, grid_for(std::max((size_t)L.n_kf, (size_t)L.n_points)), wg, 0, s, A);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipStreamSynchronize(s);
}
