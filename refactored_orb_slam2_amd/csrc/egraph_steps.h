// egraph_steps.h -- the per-item steps of Optimizer::OptimizeEssentialGraph on the device, once, for the two kernel units that run
// them: egraph_kernels.hip (one workgroup per graph: the steps of a phase separated by barriers) and egraph_grid_kernels.hip (one
// graph across the device: a phase is a launch).  Device only.  The arithmetic is egraph_internal.h's; what is stated here is which
// lane of a workgroup of EG_THREADS adds what in which order, so the two forms give the same bytes: the four interleaved partial sums
// of a tile entry and their xor 1, xor 2 combination, the 32-lane strided sums of the forward solve, the descending-row subtraction
// order of the back solve, and the incidence-list order of b and H.  No step holds a barrier unless its comment says so.
#pragma once
#include "egraph_internal.h"

#define EG_THREADS 256
#define EG_WAVES (EG_THREADS / 64)

// ---- prepare ------------------------------------------------------------------------------------------------------------------------
// the limits on vertex k and on edge e: 1 when the record breaks one
__device__ inline int eg_vertex_bad(const orbfe_eg_vertex* V, int k, bool se3) {
  const orbfe_eg_sim3 a = V[k].Scw, b = V[k].Snc;
  bool ok = eg_record_ok(a) && eg_record_ok(b);
  if (se3) ok = ok && eg_unit_scale(a.s) && eg_unit_scale(b.s);
  return ok ? 0 : 1;
}

__device__ inline int eg_edge_bad(const orbfe_eg_edge* E, int e, int n_kf) {
  const orbfe_eg_edge g = E[e];
  return (g.i >= 0 && g.i < n_kf && g.j >= 0 && g.j < n_kf && g.i != g.j && g.kind <= ORBFE_EG_LOOP_CONNECTION) ? 0 : 1;
}

// the measurement of edge e, once per edge; returns 1 when the SE3 path meets a scale beyond the tolerance
__device__ inline int eg_measure(const EgWs& W, const orbfe_eg_vertex* V, const orbfe_eg_edge* E, int e, bool se3) {
  const orbfe_eg_edge g = E[e];
  const bool loop = g.kind == ORBFE_EG_LOOP_CONNECTION;
  const OsSim3 Siw = eg_load(loop ? V[g.i].Scw : V[g.i].Snc), Sjw = eg_load(loop ? V[g.j].Scw : V[g.j].Snc);
  OsSim3 C = eg_measurement(Siw, Sjw);
  int bad = 0;
  if (se3) {
    bad = eg_unit_scale(C.s) ? 0 : 1;
    C = eg_to_se3(C);
  }
  W.meas[e] = C;
  return bad;
}

// the start estimate of vertex k, and its empty incidence count
__device__ inline void eg_vertex_init(const EgWs& W, const orbfe_eg_vertex* V, int k, bool se3) {
  const OsSim3 S = eg_load(V[k].Scw);
  W.est[k] = se3 ? eg_to_se3(S) : S;
  W.cnt[k] = 0;
  W.fill[k] = 0;
}

// edge e into the incidence lists of its two vertices; the slots are handed out in any order (integer atomics)
__device__ inline void eg_list_fill(const EgWs& W, const orbfe_eg_edge* E, int e) {
  const int i = E[e].i, j = E[e].j;
  W.list[W.start[i] + atomicAdd(&W.fill[i], 1)] = 2 * e;
  W.list[W.start[j] + atomicAdd(&W.fill[j], 1)] = 2 * e + 1;
}

// the incidence list of vertex k sorted, so its order is the edge order
__device__ inline void eg_list_sort(const EgWs& W, int k) {
  int32_t* a = W.list + W.start[k];
  const int n = W.cnt[k];
  for (int i = 1; i < n; i++) {
    const int32_t v = a[i];
    int j = i - 1;
    while (j >= 0 && a[j] > v) {
      a[j + 1] = a[j];
      j--;
    }
    a[j + 1] = v;
  }
}

// the first row block of row r's envelope: the earliest free vertex it shares an edge with (a minimum: any list order)
__device__ inline int eg_row_first(const EgWs& W, const orbfe_eg_edge* E, int r) {
  const int kf = W.kf_of_slot[r];
  int f = r;
  for (int q = W.start[kf]; q < W.start[kf + 1]; q++) {
    const int code = W.list[q];
    const int c = W.slot[(code & 1) ? E[code >> 1].i : E[code >> 1].j];
    if (c >= 0 && c < f) f = c;
  }
  return f;
}

// ---- linearise ----------------------------------------------------------------------------------------------------------------------
// the error of edge e at the estimates into err[D]
template <int D>
__device__ inline void eg_edge_error(const EgWs& W, const orbfe_eg_edge& E, int e, double* err) {
  const OsSim3 Si = W.est[E.i], Sj = W.est[E.j], C = W.meas[e];
  if constexpr (D == 7)
    eg_error_sim3(C, Si, Sj, err);
  else
    eg_error_se3(C.q, Si.q, Sj.q, err);
}

template <int D>
__device__ inline double eg_chi2(const double* err) {
  double c = 0.0;
#pragma unroll
  for (int r = 0; r < D; r++) c += err[r] * err[r];   // error . (I * error)
  return c;
}

// Column d of linearizeOplusN of a Sim3 edge for its free vertices: (e(+delta) - e(-delta)) / (2 delta) through oplus, into out
__device__ inline void eg_linearize_column(double* out, const OsSim3& C, const OsSim3& Si, const OsSim3& Sj, bool free_i, bool free_j, int d) {
  if (free_i) {
    double ep[7], em[7];
    eg_error_sim3(C, os_perturbed(Si, 1 + 2 * d, false), Sj, ep);
    eg_error_sim3(C, os_perturbed(Si, 2 + 2 * d, false), Sj, em);
#pragma unroll
    for (int r = 0; r < 7; r++) out[d * 7 + r] = os_central(ep[r], em[r]);
  }
  if (free_j) {
    double ep[7], em[7];
    eg_error_sim3(C, Si, os_perturbed(Sj, 1 + 2 * d, false), ep);
    eg_error_sim3(C, Si, os_perturbed(Sj, 2 + 2 * d, false), em);
#pragma unroll
    for (int r = 0; r < 7; r++) out[49 + d * 7 + r] = os_central(ep[r], em[r]);
  }
}

// computeError of edge e: the error into the workspace; returns chi2
template <int D>
__device__ inline double eg_linearize_error(const EgWs& W, const orbfe_eg_edge& E, int e) {
  double* out = W.je + (size_t)e * EG_EDGE_DOUBLES;
  double err[D];
  eg_edge_error<D>(W, E, e, err);
#pragma unroll
  for (int r = 0; r < D; r++) out[98 + r] = err[r];
  return eg_chi2<D>(err);
}

// computeError and linearizeOplus of edge e: the error and the Jacobians of its free vertices into the workspace; returns chi2
template <int D>
__device__ inline double eg_linearize(const EgWs& W, const orbfe_eg_edge& E, int e) {
  double* out = W.je + (size_t)e * EG_EDGE_DOUBLES;
  const OsSim3 Si = W.est[E.i], Sj = W.est[E.j], C = W.meas[e];
  const bool free_i = W.slot[E.i] >= 0, free_j = W.slot[E.j] >= 0;
  if constexpr (D == 7) {
    // linearizeOplusN, a column at a time.  A real loop: the column goes to memory
#pragma unroll 1
    for (int d = 0; d < 7; d++) eg_linearize_column(out, C, Si, Sj, free_i, free_j, d);
  } else {
    if (free_i) eg_adj(pose_mul(eg_se3_inverse(Sj.q), C.q), false, out);
    if (free_j) eg_adj(pose_mul(eg_se3_inverse(Si.q), eg_se3_inverse(C.q)), true, out + 49);
  }
  return eg_linearize_error<D>(W, E, e);
}

// the chi2 of edge e at the estimates: what a trial adds per edge
template <int D>
__device__ inline double eg_edge_chi2(const EgWs& W, const orbfe_eg_edge& E, int e) {
  double err[D];
  eg_edge_error<D>(W, E, e, err);
  return eg_chi2<D>(err);
}

// ---- build --------------------------------------------------------------------------------------------------------------------------
// the row envelope: element (a, col) of block row r, col counted from the row's first stored scalar column.  Element offsets are
// 64-bit: the envelope of the grid form exceeds 2^31 bytes
template <int D>
struct EgRow {
  double* base;
  int first, len;   // first block, scalar columns stored
  __device__ EgRow(const EgWs& W, int r) {
    first = W.first[r];
    len = (r - first + 1) * D;
    base = W.env + (size_t)W.row_off[r] * (D * D);
  }
  __device__ double* row(int a) const { return base + (size_t)a * len; }
};

// b of row block r, entry k: the sum over the vertex's edges of J^T (-e)
template <int D>
__device__ inline double eg_b_entry(const EgWs& W, int r, int k) {
  const int kf = W.kf_of_slot[r];
  double s = 0.0;
  for (int q = W.start[kf]; q < W.start[kf + 1]; q++) {
    const int code = W.list[q];
    const double* je = W.je + (size_t)(code >> 1) * EG_EDGE_DOUBLES;
    const double* J = je + (code & 1) * 49 + k * D;
    double g = 0.0;
#pragma unroll
    for (int m = 0; m < D; m++) g += J[m] * (-je[98 + m]);
    s += g;
  }
  return s;
}

// Entry (k, l) of every block of row r that an edge of the vertex touches: the diagonal block (with lambda on its diagonal) and, for
// an edge whose other vertex lies before r, that block.  The envelope was zeroed before
template <int D>
__device__ inline void eg_h_entries(const EgWs& W, const orbfe_eg_edge* E, int r, int k, int l, double lambda) {
  const int kf = W.kf_of_slot[r];
  const EgRow<D> Rr(W, r);
  double diag = 0.0;
  for (int q = W.start[kf]; q < W.start[kf + 1]; q++) {
    const int code = W.list[q], e = code >> 1, side = code & 1;
    const double* je = W.je + (size_t)e * EG_EDGE_DOUBLES;
    const double* Jr = je + side * 49 + k * D;
    const double* Jd = je + side * 49 + l * D;
    double h = 0.0;
#pragma unroll
    for (int m = 0; m < D; m++) h += Jr[m] * Jd[m];
    diag += h;
    const int c = W.slot[side ? E[e].i : E[e].j];
    if (c >= 0 && c < r) {
      const double* Jc = je + (1 - side) * 49 + l * D;
      double g = 0.0;
#pragma unroll
      for (int m = 0; m < D; m++) g += Jr[m] * Jc[m];
      double* o = Rr.row(k) + (c - Rr.first) * D + l;
      *o = *o + g;
    }
  }
  Rr.row(k)[(r - Rr.first) * D + l] = k == l ? diag + lambda : diag;
}

// ---- factor: block L L^T of the envelope, up-looking --------------------------------------------------------------------------------
// Sum of the workgroup's 4 * D * D dot-product lanes: entry (a, b) of `target` minus rowa[a][0 .. n) . rowb[b][0 .. n) into tile[49]
template <int D>
__device__ inline void eg_tile(double* tile, const double* pa, size_t stride_a, const double* pb, size_t stride_b, int n, const double* target,
                               size_t stride_t) {
  const int tid = threadIdx.x, ent = tid >> 2, q = tid & 3;
  const bool mine = ent < D * D;
  const int a = mine ? ent / D : 0, b = mine ? ent % D : 0;
  double s = 0.0;
  if (mine) {
    const double* ra = pa + a * stride_a;
    const double* rb = pb + b * stride_b;
    for (int m = q; m < n; m += 4) s += ra[m] * rb[m];
  }
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if (mine && q == 0) tile[ent] = target[a * stride_t + b] - s;
}

// the tile of block (r, c), c < r: A_rc minus the dot products of the two rows' stored parts before c
template <int D>
__device__ inline void eg_tile_offdiag(double* tile, const EgRow<D>& Rr, const EgRow<D>& Rc, int c) {
  const int ks = Rr.first > Rc.first ? Rr.first : Rc.first;
  eg_tile<D>(tile, Rr.base + (ks - Rr.first) * D, Rr.len, Rc.base + (ks - Rc.first) * D, Rc.len, (c - ks) * D,
             Rr.base + (c - Rr.first) * D, Rr.len);
}

// the tile of the diagonal block of row r
template <int D>
__device__ inline void eg_tile_diag(double* tile, const EgRow<D>& Rr, int r) {
  eg_tile<D>(tile, Rr.base, Rr.len, Rr.base, Rr.len, (r - Rr.first) * D, Rr.base + (r - Rr.first) * D, Rr.len);
}

// lane `a` < D, behind the barrier after eg_tile_offdiag: row a of block (r, c) is x with x L_cc^T = tile row a
template <int D>
__device__ inline void eg_block_solve(const double* tile, const EgRow<D>& Rr, const EgRow<D>& Rc, int c, int a) {
  const double* Lcc = Rc.base + (c - Rc.first) * D;
  double x[D];
#pragma unroll
  for (int b = 0; b < D; b++) {
    double s = tile[a * D + b];
#pragma unroll
    for (int m = 0; m < b; m++) s -= x[m] * Lcc[(size_t)b * Rc.len + m];
    x[b] = s / Lcc[(size_t)b * Rc.len + b];
  }
  double* o = Rr.row(a) + (c - Rr.first) * D;
#pragma unroll
  for (int b = 0; b < D; b++) o[b] = x[b];
}

// one lane, behind the barrier after eg_tile_diag: the D x D Cholesky of the diagonal block of row r; false when a pivot is not > 0
template <int D>
__device__ inline bool eg_diag_cholesky(const double* tile, const EgRow<D>& Rr, int r) {
  double Lm[D][D];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < D; j++) {
    double d = tile[j * D + j];
#pragma unroll
    for (int k = 0; k < j; k++) d -= Lm[j][k] * Lm[j][k];
    if (!(d > 0.0)) ok = false;
    const double ljj = sqrt(d);
    Lm[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < D; i++) {
      double s = tile[i * D + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= Lm[i][k] * Lm[j][k];
      Lm[i][j] = s / ljj;
    }
  }
  double* o = Rr.base + (r - Rr.first) * D;
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) o[(size_t)i * Rr.len + j] = Lm[i][j];
  return ok;
}

// ---- solve: one workgroup of EG_THREADS, every lane calls it ------------------------------------------------------------------------
// L y = b, then L^T x = y; W.y holds b on entry and x on return; v: 8 doubles of LDS.  Forward by rows (32 lanes per scalar row of
// the block), backward by columns (a lane per element of the row).  Ends behind a barrier
template <int D>
__device__ inline void eg_solve(const EgWs& W, double* v, int nf) {
  const int tid = threadIdx.x;
  for (int r = 0; r < nf; r++) {
    const EgRow<D> Rr(W, r);
    const int n = (r - Rr.first) * D, a = tid >> 5, q = tid & 31;
    double s = 0.0;
    if (a < D) {
      const double* row = Rr.row(a);
      const double* y = W.y + (size_t)Rr.first * D;
      for (int m = q; m < n; m += 32) s += row[m] * y[m];
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (a < D && q == 0) v[a] = W.y[(size_t)r * D + a] - s;
    __syncthreads();
    if (tid == 0) {
      const double* Lrr = Rr.base + n;
      double y[D];
#pragma unroll
      for (int i = 0; i < D; i++) {
        double t = v[i];
#pragma unroll
        for (int m = 0; m < i; m++) t -= Lrr[(size_t)i * Rr.len + m] * y[m];
        y[i] = t / Lrr[(size_t)i * Rr.len + i];
      }
#pragma unroll
      for (int i = 0; i < D; i++) W.y[(size_t)r * D + i] = y[i];
    }
    __syncthreads();
  }
  for (int r = nf - 1; r >= 0; r--) {
    const EgRow<D> Rr(W, r);
    const int n = (r - Rr.first) * D;
    if (tid == 0) {
      const double* Lrr = Rr.base + n;
      double x[D];
#pragma unroll
      for (int i = D - 1; i >= 0; i--) {
        double t = W.y[(size_t)r * D + i];
#pragma unroll
        for (int m = i + 1; m < D; m++) t -= Lrr[(size_t)m * Rr.len + i] * x[m];
        x[i] = t / Lrr[(size_t)i * Rr.len + i];
      }
#pragma unroll
      for (int i = 0; i < D; i++) {
        W.y[(size_t)r * D + i] = x[i];
        v[i] = x[i];
      }
    }
    __syncthreads();
    double* y = W.y + (size_t)Rr.first * D;
    for (int m = tid; m < n; m += EG_THREADS) {
      double t = y[m];
#pragma unroll
      for (int i = 0; i < D; i++) t -= Rr.base[(size_t)i * Rr.len + m] * v[i];
      y[m] = t;
    }
    __syncthreads();
  }
}

// ---- trial --------------------------------------------------------------------------------------------------------------------------
// computeScale's term of scalar row t of the update
__device__ inline double eg_scale_term(const EgWs& W, int t, double lambda) { return W.y[t] * (lambda * W.y[t] + W.b[t]); }

// push and oplus of row block r
template <int D>
__device__ inline void eg_push_oplus(const EgWs& W, int r) {
  const int kf = W.kf_of_slot[r];
  const OsSim3 S = W.est[kf];
  W.bak[kf] = S;
  double x[D];
#pragma unroll
  for (int m = 0; m < D; m++) x[m] = W.y[(size_t)r * D + m];
  if constexpr (D == 6)
    W.est[kf] = eg_oplus_se3(S, x);
  else
    W.est[kf] = os_oplus(S, x, false);
}

// pop of row block r
__device__ inline void eg_pop(const EgWs& W, int r) {
  const int kf = W.kf_of_slot[r];
  W.est[kf] = W.bak[kf];
}

// ---- write-back ---------------------------------------------------------------------------------------------------------------------
// the records of a problem that did not run, or of its vertices that are not in the system: Scw as given, and its pose
__device__ inline void eg_write_through(const orbfe_eg_vertex* V, int k, bool se3, orbfe_eg_sim3* sim3_out, float* poses_out) {
  const orbfe_eg_sim3 S = V[k].Scw;
  sim3_out[k] = S;
  float T[12];
  eg_pose_row(eg_load(S), se3, T);
#pragma unroll
  for (int j = 0; j < 12; j++) poses_out[(size_t)k * 12 + j] = T[j];
}

// vertex k of a problem that ran: its estimate when it is in the system, else written through
__device__ inline void eg_write_vertex(const EgWs& W, const orbfe_eg_vertex* V, int k, bool se3, orbfe_eg_sim3* sim3_out, float* poses_out) {
  if (W.slot[k] < 0) {
    eg_write_through(V, k, se3, sim3_out, poses_out);
  } else {
    const OsSim3 S = W.est[k];
    orbfe_eg_sim3 o;
    eg_store(S, o);
    sim3_out[k] = o;
    float T[12];
    eg_pose_row(S, se3, T);
#pragma unroll
    for (int j = 0; j < 12; j++) poses_out[(size_t)k * 12 + j] = T[j];
  }
}

// the record of a problem before anything of it ran
__device__ inline orbfe_eg_result eg_result_refused(int n_edges) {
  orbfe_eg_result res;
  res.status = ORBFE_EG_REFUSED;
  res.iterations = 0;
  res.trials = 0;
  res.n_free = 0;
  res.n_edges = n_edges;
  res.envelope_blocks = 0;
  res.chi2_first = 0.0;
  res.chi2_last = 0.0;
  res.lambda = 0.0;
  return res;
}
