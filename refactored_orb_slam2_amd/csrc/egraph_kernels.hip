// egraph_kernels.hip -- Optimizer::OptimizeEssentialGraph (L/src/Optimizer.cc:1366) for a batch of pose graphs, and the map
// correction behind it.  The arithmetic is egraph_internal.h's, one item per call; the Levenberg rules are lm_internal.h's; what is
// stated here is who does which item and where the barriers are.
//
// One workgroup of 256 threads per problem, templated on the dimension D of a vertex: 7 (VertexSim3Expmap, numeric Jacobians) or 6
// (VertexSE3Expmap, analytic ones).  Everything that grows with the graph is the problem's workspace in HBM; LDS holds the reduction
// buffers and one D x D tile.  Every sum has ONE owner who walks a sorted list, so no floating-point atomics exist and a problem's
// bytes depend on nothing but its own rows:
//   prepare    a lane per record for the limits and the measurements; the incidence lists by integer atomics (counts and slots),
//              then sorted per vertex so their order is the edge order; the row blocks, the first block of every row's envelope and
//              the row offsets in vertex order
//   linearise  a lane per edge: the error, chi2 and the Jacobians of its free vertices into the workspace, a column at a time
//   build      a lane per (row block, entry): b, and H + lambda I into the envelope -- the diagonal block and, for every edge whose
//              other vertex lies before the row, that block of the row
//   factor     block L L^T row by row (up-looking): block (r, c) is A_rc minus the dot products of the two rows' stored parts -- each
//              a contiguous run, four lanes per entry -- through an LDS tile and D lanes' triangular solve against L_cc; the diagonal
//              block the same with one lane's D x D Cholesky.  Two barriers per block.  A pivot that is not > 0 ends it
//   solve      forward by rows (32 lanes per scalar row of the block), backward by columns (a lane per element of the row)
//   trial      a lane per row block for oplus, a lane per edge for the trial's chi2
//   control    chi2 and computeScale land in LDS (lm_reduce.h); each lane repeats the Levenberg bookkeeping on those identical
//              values, so control flow is uniform over the workgroup by construction
#include "egraph_internal.h"
#include "lm_reduce.h"

#define EG_THREADS 256
#define EG_WAVES (EG_THREADS / 64)

struct EgShared {
  double red[EG_WAVES * 2], tot[2];
  double tile[49];
  double v[8];
  int red_i[EG_WAVES];
  int n_free, total, fail;
};

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

// computeError and linearizeOplus of edge e: the error and the Jacobians of its free vertices into the workspace; returns chi2
template <int D>
__device__ inline double eg_linearize(const EgWs& W, const orbfe_eg_edge& E, int e) {
  double* out = W.je + (size_t)e * EG_EDGE_DOUBLES;
  const OsSim3 Si = W.est[E.i], Sj = W.est[E.j], C = W.meas[e];
  const bool free_i = W.slot[E.i] >= 0, free_j = W.slot[E.j] >= 0;
  double err[D];
  if constexpr (D == 7) {
    eg_error_sim3(C, Si, Sj, err);
    // linearizeOplusN: column d = (e(+delta) - e(-delta)) / (2 delta) through oplus.  A real loop: the column goes to memory
#pragma unroll 1
    for (int d = 0; d < 7; d++) {
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
  } else {
    eg_error_se3(C.q, Si.q, Sj.q, err);
    if (free_i) eg_adj(pose_mul(eg_se3_inverse(Sj.q), C.q), false, out);
    if (free_j) eg_adj(pose_mul(eg_se3_inverse(Si.q), eg_se3_inverse(C.q)), true, out + 49);
  }
#pragma unroll
  for (int r = 0; r < D; r++) out[98 + r] = err[r];
  return eg_chi2<D>(err);
}

// the row envelope: element (a, col) of block row r, col counted from the row's first stored scalar column
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

// Sum of the workgroup's 4 * D * D dot-product lanes: entry (a, b) of `target` minus rowa[a][0 .. n) . rowb[b][0 .. n) into the tile
template <int D>
__device__ inline void eg_tile(EgShared& sh, const double* pa, size_t stride_a, const double* pb, size_t stride_b, int n, const double* target,
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
  if (mine && q == 0) sh.tile[ent] = target[a * stride_t + b] - s;
}

// In-place block L L^T of the envelope.  Uniform; returns false when a pivot is not > 0.  Ends behind a barrier
template <int D>
__device__ inline bool eg_factor(const EgWs& W, EgShared& sh, int nf) {
  const int tid = threadIdx.x;
  if (tid == 0) sh.fail = 0;
  __syncthreads();
  for (int r = 0; r < nf; r++) {
    const EgRow<D> Rr(W, r);
    for (int c = Rr.first; c < r; c++) {
      const EgRow<D> Rc(W, c);
      const int ks = Rr.first > Rc.first ? Rr.first : Rc.first;
      eg_tile<D>(sh, Rr.base + (ks - Rr.first) * D, Rr.len, Rc.base + (ks - Rc.first) * D, Rc.len, (c - ks) * D,
                 Rr.base + (c - Rr.first) * D, Rr.len);
      __syncthreads();
      if (tid < D) {   // row tid of the block: x L_cc^T = tile row
        const double* Lcc = Rc.base + (c - Rc.first) * D;
        double x[D];
#pragma unroll
        for (int b = 0; b < D; b++) {
          double s = sh.tile[tid * D + b];
#pragma unroll
          for (int m = 0; m < b; m++) s -= x[m] * Lcc[(size_t)b * Rc.len + m];
          x[b] = s / Lcc[(size_t)b * Rc.len + b];
        }
        double* o = Rr.row(tid) + (c - Rr.first) * D;
#pragma unroll
        for (int b = 0; b < D; b++) o[b] = x[b];
      }
      __syncthreads();
    }
    eg_tile<D>(sh, Rr.base, Rr.len, Rr.base, Rr.len, (r - Rr.first) * D, Rr.base + (r - Rr.first) * D, Rr.len);
    __syncthreads();
    if (tid == 0) {   // the D x D Cholesky of the diagonal block
      double Lm[D][D];
      bool ok = true;
#pragma unroll
      for (int j = 0; j < D; j++) {
        double d = sh.tile[j * D + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= Lm[j][k] * Lm[j][k];
        if (!(d > 0.0)) ok = false;
        const double ljj = sqrt(d);
        Lm[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < D; i++) {
          double s = sh.tile[i * D + j];
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
      if (!ok) sh.fail = 1;
    }
    __syncthreads();
    if (sh.fail) return false;   // uniform: every lane reads the same word behind the barrier
  }
  return true;
}

// L y = b, then L^T x = y; W.y holds b on entry and x on return.  Ends behind a barrier
template <int D>
__device__ inline void eg_solve(const EgWs& W, EgShared& sh, int nf) {
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
    if (a < D && q == 0) sh.v[a] = W.y[(size_t)r * D + a] - s;
    __syncthreads();
    if (tid == 0) {
      const double* Lrr = Rr.base + n;
      double y[D];
#pragma unroll
      for (int i = 0; i < D; i++) {
        double t = sh.v[i];
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
        sh.v[i] = x[i];
      }
    }
    __syncthreads();
    double* y = W.y + (size_t)Rr.first * D;
    for (int m = tid; m < n; m += EG_THREADS) {
      double t = y[m];
#pragma unroll
      for (int i = 0; i < D; i++) t -= Rr.base[(size_t)i * Rr.len + m] * sh.v[i];
      y[m] = t;
    }
    __syncthreads();
  }
}

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

// the records of a problem that did not run, or of its vertices that are not in the system: Scw as given, and its pose
__device__ inline void eg_write_through(const orbfe_eg_vertex* V, int k, bool se3, orbfe_eg_sim3* sim3_out, float* poses_out) {
  const orbfe_eg_sim3 S = V[k].Scw;
  sim3_out[k] = S;
  float T[12];
  eg_pose_row(eg_load(S), se3, T);
#pragma unroll
  for (int j = 0; j < 12; j++) poses_out[(size_t)k * 12 + j] = T[j];
}

template <int D>
__global__ __launch_bounds__(EG_THREADS) void essential_graph_kernel(EgLaunch L) {
  __shared__ EgShared sh;
  constexpr bool SE3 = D == 6;
  const int tid = threadIdx.x;
  const orbfe_eg_problem Q = L.problems[blockIdx.x];
  orbfe_eg_result res;
  res.status = ORBFE_EG_REFUSED;
  res.iterations = 0;
  res.trials = 0;
  res.n_free = 0;
  res.n_edges = Q.n_edges;
  res.envelope_blocks = 0;
  res.chi2_first = 0.0;
  res.chi2_last = 0.0;
  res.lambda = 0.0;
  if (Q.n_kf < 0 || Q.n_kf > L.kf_cap || Q.n_edges < 0 || Q.n_edges > L.edge_cap || Q.kf_offset < 0 || Q.edge_offset < 0) {
    if (tid == 0) L.result[blockIdx.x] = res;   // nothing of such a problem can be addressed
    return;
  }
  EgWs W;
  eg_ws_carve(L.workspace + (size_t)blockIdx.x * eg_ws_bytes(L.kf_cap, L.edge_cap, L.env_cap), L.kf_cap, L.edge_cap, L.env_cap, W);
  const int n_kf = Q.n_kf, n_e = Q.n_edges;
  const orbfe_eg_vertex* V = L.vertices + Q.kf_offset;
  const orbfe_eg_edge* E = L.edges + Q.edge_offset;
  orbfe_eg_sim3* sim3_out = L.sim3_out + Q.kf_offset;
  float* poses_out = L.poses_out + (size_t)Q.kf_offset * 12;

  // the limits
  int bad = 0;
  for (int k = tid; k < n_kf; k += EG_THREADS) {
    const orbfe_eg_sim3 a = V[k].Scw, b = V[k].Snc;
    bool ok = eg_record_ok(a) && eg_record_ok(b);
    if (SE3) ok = ok && eg_unit_scale(a.s) && eg_unit_scale(b.s);
    bad += ok ? 0 : 1;
  }
  for (int e = tid; e < n_e; e += EG_THREADS) {
    const orbfe_eg_edge g = E[e];
    bad += (g.i >= 0 && g.i < n_kf && g.j >= 0 && g.j < n_kf && g.i != g.j && g.kind <= ORBFE_EG_LOOP_CONNECTION) ? 0 : 1;
  }
  bad = lm_reduce_count<EG_WAVES>(bad, sh.red_i, tid);
  if (bad == 0) {   // uniform.  The measurements, once per edge
    for (int e = tid; e < n_e; e += EG_THREADS) {
      const orbfe_eg_edge g = E[e];
      const bool loop = g.kind == ORBFE_EG_LOOP_CONNECTION;
      const OsSim3 Siw = eg_load(loop ? V[g.i].Scw : V[g.i].Snc), Sjw = eg_load(loop ? V[g.j].Scw : V[g.j].Snc);
      OsSim3 C = eg_measurement(Siw, Sjw);
      if (SE3) {
        bad += eg_unit_scale(C.s) ? 0 : 1;
        C = eg_to_se3(C);
      }
      W.meas[e] = C;
    }
    bad = lm_reduce_count<EG_WAVES>(bad, sh.red_i, tid);
  }
  if (bad) {
    for (int k = tid; k < n_kf; k += EG_THREADS) eg_write_through(V, k, SE3, sim3_out, poses_out);
    if (tid == 0) L.result[blockIdx.x] = res;
    return;
  }

  // the estimates; the incidence lists
  for (int k = tid; k < n_kf; k += EG_THREADS) {
    const OsSim3 S = eg_load(V[k].Scw);
    W.est[k] = SE3 ? eg_to_se3(S) : S;
    W.cnt[k] = 0;
    W.fill[k] = 0;
  }
  __syncthreads();
  for (int e = tid; e < n_e; e += EG_THREADS) {
    atomicAdd(&W.cnt[E[e].i], 1);
    atomicAdd(&W.cnt[E[e].j], 1);
  }
  __syncthreads();
  if (tid == 0) {   // vertex order is elimination order
    int o = 0, nf = 0;
    for (int k = 0; k < n_kf; k++) {
      W.start[k] = o;
      o += W.cnt[k];
      if (!V[k].fixed && W.cnt[k] > 0) {
        W.kf_of_slot[nf] = k;
        W.slot[k] = nf++;
      } else {
        W.slot[k] = -1;
      }
    }
    W.start[n_kf] = o;
    sh.n_free = nf;
  }
  __syncthreads();
  const int nf = sh.n_free;
  res.n_free = nf;
  if (nf == 0 || n_e == 0) {   // uniform: optimize() has nothing to do
    res.status = ORBFE_EG_DONE;
    for (int k = tid; k < n_kf; k += EG_THREADS) eg_write_through(V, k, SE3, sim3_out, poses_out);
    if (tid == 0) L.result[blockIdx.x] = res;
    return;
  }
  for (int e = tid; e < n_e; e += EG_THREADS) {
    const int i = E[e].i, j = E[e].j;
    W.list[W.start[i] + atomicAdd(&W.fill[i], 1)] = 2 * e;
    W.list[W.start[j] + atomicAdd(&W.fill[j], 1)] = 2 * e + 1;
  }
  __syncthreads();
  for (int k = tid; k < n_kf; k += EG_THREADS) {   // the slots were handed out in any order: sort, so a list is in edge order
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
  __syncthreads();
  for (int r = tid; r < nf; r += EG_THREADS) {
    const int kf = W.kf_of_slot[r];
    int f = r;
    for (int q = W.start[kf]; q < W.start[kf + 1]; q++) {
      const int code = W.list[q];
      const int c = W.slot[(code & 1) ? E[code >> 1].i : E[code >> 1].j];
      if (c >= 0 && c < f) f = c;
    }
    W.first[r] = f;
  }
  __syncthreads();
  if (tid == 0) {
    long long o = 0;
    for (int r = 0; r < nf; r++) {
      W.row_off[r] = (int32_t)(o < 0x7fffffff ? o : 0x7fffffff);
      o += r - W.first[r] + 1;
    }
    sh.total = (int)(o < 0x7fffffff ? o : 0x7fffffff);
  }
  __syncthreads();
  const int total = sh.total;
  res.envelope_blocks = total;
  if (total > L.env_cap) {   // uniform
    for (int k = tid; k < n_kf; k += EG_THREADS) eg_write_through(V, k, SE3, sim3_out, poses_out);
    if (tid == 0) L.result[blockIdx.x] = res;
    return;
  }
  res.status = ORBFE_EG_DONE;

  // optimize(20)
  const int n = nf * D;
  LmState lm;
  lm.lambda = EG_LAMBDA_INIT;
  lm.ni = 2.0;
  double current_chi = 0.0;
  for (int it = 0; it < EG_ITERATIONS; it++) {
    double v[2] = {0.0, 0.0};
    for (int e = tid; e < n_e; e += EG_THREADS) v[0] += eg_linearize<D>(W, E[e], e);
    lm_reduce<1, 2, EG_WAVES>(v, sh.red, sh.tot, tid);   // its barriers also publish the Jacobians
    current_chi = sh.tot[0];
    if (it == 0) res.chi2_first = current_chi;
    for (int t = tid; t < n; t += EG_THREADS) W.b[t] = eg_b_entry<D>(W, t / D, t % D);
    double rho = 0.0;
    int qmax = 0;
    do {
      const double lambda = lm.lambda;
      for (int t = tid; t < total * (D * D); t += EG_THREADS) W.env[t] = 0.0;
      for (int t = tid; t < n; t += EG_THREADS) W.y[t] = W.b[t];
      __syncthreads();
      for (int t = tid; t < nf * (D * D); t += EG_THREADS) eg_h_entries<D>(W, E, t / (D * D), (t % (D * D)) / D, t % D, lambda);
      __syncthreads();
      const bool ok2 = eg_factor<D>(W, sh, nf);
      double temp_chi = 0.0, scale = 0.0;
      if (ok2) {   // uniform
        eg_solve<D>(W, sh, nf);
        double u[2] = {0.0, 0.0};
        for (int t = tid; t < n; t += EG_THREADS) u[1] += W.y[t] * (lambda * W.y[t] + W.b[t]);   // computeScale
        for (int r = tid; r < nf; r += EG_THREADS) {   // push, oplus
          const int kf = W.kf_of_slot[r];
          const OsSim3 S = W.est[kf];
          W.bak[kf] = S;
          double x[D];
#pragma unroll
          for (int m = 0; m < D; m++) x[m] = W.y[(size_t)r * D + m];
          if constexpr (SE3)
            W.est[kf] = eg_oplus_se3(S, x);
          else
            W.est[kf] = os_oplus(S, x, false);
        }
        __syncthreads();
        for (int e = tid; e < n_e; e += EG_THREADS) {
          double err[D];
          eg_edge_error<D>(W, E[e], e, err);
          u[0] += eg_chi2<D>(err);
        }
        lm_reduce<2, 2, EG_WAVES>(u, sh.red, sh.tot, tid);
        temp_chi = sh.tot[0];
        scale = sh.tot[1];
      } else {
        res.status = ORBFE_EG_FACTOR_FAILED;
      }
      res.trials++;
      if (lm_trial_scaled(lm, ok2, current_chi, temp_chi, scale, &rho)) {
        current_chi = temp_chi;
      } else {
        if (ok2)   // pop
          for (int r = tid; r < nf; r += EG_THREADS) {
            const int kf = W.kf_of_slot[r];
            W.est[kf] = W.bak[kf];
          }
        if (!isfinite(lm.lambda)) break;
      }
      __syncthreads();
      qmax++;
    } while (rho < 0 && qmax < 10);
    __syncthreads();
    res.iterations++;
    if (qmax == 10 || rho == 0 || !isfinite(lm.lambda)) break;   // Terminate
  }
  res.chi2_last = current_chi;
  res.lambda = lm.lambda;
  for (int k = tid; k < n_kf; k += EG_THREADS) {
    if (W.slot[k] < 0) {
      eg_write_through(V, k, SE3, sim3_out, poses_out);
    } else {
      const OsSim3 S = W.est[k];
      orbfe_eg_sim3 o;
      eg_store(S, o);
      sim3_out[k] = o;
      float T[12];
      eg_pose_row(S, SE3, T);
#pragma unroll
      for (int j = 0; j < 12; j++) poses_out[(size_t)k * 12 + j] = T[j];
    }
  }
  if (tid == 0) L.result[blockIdx.x] = res;
}

void orbfe_launch_essential_graph(const EgLaunch& L, int P, hipStream_t s) {
  if (P < 1) return;
  if (L.flags & ORBFE_EG_FIX_SCALE)
    hipLaunchKernelGGL(essential_graph_kernel<6>, dim3(P), dim3(EG_THREADS), 0, s, L);
  else
    hipLaunchKernelGGL(essential_graph_kernel<7>, dim3(P), dim3(EG_THREADS), 0, s, L);
}

// One thread per point, any grid size
__global__ __launch_bounds__(256) void sim3_correct_points_kernel(const float* points, int n, const int32_t* ref, const uint8_t* from,
                                                                  int from_stride, const orbfe_eg_sim3* to, int n_tables, float* out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
    const float P3[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
    const int r = ref[p];
    float o[3] = {P3[0], P3[1], P3[2]};
    if (r >= 0 && r < n_tables) {
      const orbfe_eg_sim3 a = *reinterpret_cast<const orbfe_eg_sim3*>(from + (size_t)r * from_stride), b = to[r];
      eg_correct_point(eg_load(a), eg_load(b), P3, o);
    }
    out[3 * p] = o[0];
    out[3 * p + 1] = o[1];
    out[3 * p + 2] = o[2];
  }
}

void orbfe_launch_correct_points(const float* points, int n, const int32_t* ref, const uint8_t* from, int from_stride,
                                 const orbfe_eg_sim3* to, int n_tables, float* out, hipStream_t s) {
  if (n < 1) return;
  const int blocks = (n + 255) / 256;
  hipLaunchKernelGGL(sim3_correct_points_kernel, dim3(blocks < 65535 ? blocks : 65535), dim3(256), 0, s, points, n, ref, from, from_stride,
                     to, n_tables, out);
}
