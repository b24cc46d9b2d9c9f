// egraph_kernels.hip -- Optimizer::OptimizeEssentialGraph (L/src/Optimizer.cc:1366) for a batch of pose graphs, and the map
// correction behind it.  The arithmetic is egraph_internal.h's, one item per call; the per-item steps -- which lane adds what in
// which order -- are egraph_steps.h's, shared with the form of one graph across the device (egraph_grid_kernels.hip); the Levenberg
// rules are lm_internal.h's; what is stated here is who does which item and where the barriers are.
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
#include "egraph_steps.h"
#include "lm_reduce.h"

struct EgShared {
  double red[EG_WAVES * 2], tot[2];
  double tile[49];
  double v[8];
  int red_i[EG_WAVES];
  int n_free, total, fail;
};

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
      eg_tile_offdiag<D>(sh.tile, Rr, Rc, c);
      __syncthreads();
      if (tid < D) eg_block_solve<D>(sh.tile, Rr, Rc, c, tid);
      __syncthreads();
    }
    eg_tile_diag<D>(sh.tile, Rr, r);
    __syncthreads();
    if (tid == 0 && !eg_diag_cholesky<D>(sh.tile, Rr, r)) sh.fail = 1;
    __syncthreads();
    if (sh.fail) return false;   // uniform: every lane reads the same word behind the barrier
  }
  return true;
}

template <int D>
__global__ __launch_bounds__(EG_THREADS) void essential_graph_kernel(EgLaunch L) {
  __shared__ EgShared sh;
  constexpr bool SE3 = D == 6;
  const int tid = threadIdx.x;
  const orbfe_eg_problem Q = L.problems[blockIdx.x];
  orbfe_eg_result res = eg_result_refused(Q.n_edges);
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
  for (int k = tid; k < n_kf; k += EG_THREADS) bad += eg_vertex_bad(V, k, SE3);
  for (int e = tid; e < n_e; e += EG_THREADS) bad += eg_edge_bad(E, e, n_kf);
  bad = lm_reduce_count<EG_WAVES>(bad, sh.red_i, tid);
  if (bad == 0) {   // uniform.  The measurements, once per edge
    for (int e = tid; e < n_e; e += EG_THREADS) bad += eg_measure(W, V, E, e, SE3);
    bad = lm_reduce_count<EG_WAVES>(bad, sh.red_i, tid);
  }
  if (bad) {
    for (int k = tid; k < n_kf; k += EG_THREADS) eg_write_through(V, k, SE3, sim3_out, poses_out);
    if (tid == 0) L.result[blockIdx.x] = res;
    return;
  }

  // the estimates; the incidence lists
  for (int k = tid; k < n_kf; k += EG_THREADS) eg_vertex_init(W, V, k, SE3);
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
  for (int e = tid; e < n_e; e += EG_THREADS) eg_list_fill(W, E, e);
  __syncthreads();
  for (int k = tid; k < n_kf; k += EG_THREADS) eg_list_sort(W, k);   // the slots were handed out in any order: sort, so a list is in edge order
  __syncthreads();
  for (int r = tid; r < nf; r += EG_THREADS) W.first[r] = eg_row_first(W, E, r);
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
        eg_solve<D>(W, sh.v, nf);
        double u[2] = {0.0, 0.0};
        for (int t = tid; t < n; t += EG_THREADS) u[1] += eg_scale_term(W, t, lambda);   // computeScale
        for (int r = tid; r < nf; r += EG_THREADS) eg_push_oplus<D>(W, r);
        __syncthreads();
        for (int e = tid; e < n_e; e += EG_THREADS) u[0] += eg_edge_chi2<D>(W, E[e], e);
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
          for (int r = tid; r < nf; r += EG_THREADS) eg_pop(W, r);
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
  for (int k = tid; k < n_kf; k += EG_THREADS) eg_write_vertex(W, V, k, SE3, sim3_out, poses_out);
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
