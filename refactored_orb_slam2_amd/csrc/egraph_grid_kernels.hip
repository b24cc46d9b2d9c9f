// egraph_grid_kernels.hip -- Optimizer::OptimizeEssentialGraph (L/src/Optimizer.cc:1366) for ONE graph across the whole device.
// egraph_kernels.hip gives a graph one workgroup, which walks the blocks of the row envelope one after the other; here every phase
// of a trial is a launch over the grid and the launch boundary is the only grid-wide synchronisation: no grid barrier, no cooperative
// launch, no flag anybody spins on, every device loop bounded by a count known at its launch.  The per-item steps are
// egraph_steps.h's, called with the same items in the same order, so a graph both forms take gives the same bytes:
//   prepare    a lane per record for the limits, the start estimates and the measurements; the incidence lists by integer atomics,
//              sorted per vertex; one workgroup hands out the slots and the row offsets in vertex order (as the one workgroup's
//              lane 0 does)
//   plan       on the HOST, once per call: first[] comes down (n_free ints), the blocks sorted by level go up
//              (egraph_grid_internal.h: eg_level_plan)
//   linearise  a lane per edge (Sim3: per edge and column of the numeric Jacobian); its chi2 into chi[]; b: a lane per scalar row
//   build      a lane per element zeroes the envelope; a lane per (row block, entry) writes H + lambda I
//   factor     ONE LAUNCH PER LEVEL, a workgroup per block of that level: eg_tile with its four lanes per entry, then the D-lane
//              solve against L_cc, or one lane's Cholesky for a diagonal block.  Every block whose inputs are complete is in flight.
//              A pivot that is not > 0 sets a fail word; every later launch of the trial returns at once on it
//   solve      one workgroup, one launch: eg_solve as it is.  Its cost grows with rows, not blocks
//   trial      a lane per row block for push / oplus, a lane per edge for the trial's chi2 into chi[]
//   control    one workgroup: lane tid sums items tid, tid + 256, ... of chi[] and of computeScale -- what the one workgroup's lane
//              would have added, in its order --, lm_reduce.h unchanged, then lane 0 runs lm_internal.h's bookkeeping and leaves the
//              control record the host reads once per trial
#include <algorithm>

#include "egraph_grid_internal.h"
#include "egraph_steps.h"
#include "lm_reduce.h"

struct EgridArgs {
  EgridLaunch L;
  EgridWs G;
};

// a pivot of this trial was not > 0: read behind the factorisation's last launch
__device__ inline bool egrid_failed(const EgridArgs& A) { return (A.G.dev->fail[0] | A.G.dev->fail[1]) != 0; }

__device__ inline size_t egrid_gid() { return (size_t)blockIdx.x * EG_THREADS + threadIdx.x; }

// ---- prepare ------------------------------------------------------------------------------------------------------------------------
// dev was zeroed by the host.  The limits on every record; the start estimates and empty counts
__global__ __launch_bounds__(EG_THREADS) void egrid_check(EgridArgs A) {
  const bool se3 = (A.L.flags & ORBFE_EG_FIX_SCALE) != 0;
  const size_t g = egrid_gid();
  int bad = 0;
  if (g < (size_t)A.L.n_kf) {
    bad += eg_vertex_bad(A.L.vertices, (int)g, se3);
    eg_vertex_init(A.G.W, A.L.vertices, (int)g, se3);
  }
  if (g < (size_t)A.L.n_edges) bad += eg_edge_bad(A.L.edges, (int)g, A.L.n_kf);
  if (bad) A.G.dev->bad = 1;
}

// the measurements, once per edge, and the edges at every vertex (integer atomics)
__global__ __launch_bounds__(EG_THREADS) void egrid_measure(EgridArgs A) {
  if (A.G.dev->bad) return;   // an edge may name a vertex that does not exist
  const size_t e = egrid_gid();
  if (e >= (size_t)A.L.n_edges) return;
  if (eg_measure(A.G.W, A.L.vertices, A.L.edges, (int)e, (A.L.flags & ORBFE_EG_FIX_SCALE) != 0)) A.G.dev->bad = 1;
  atomicAdd(&A.G.W.cnt[A.L.edges[e].i], 1);
  atomicAdd(&A.G.W.cnt[A.L.edges[e].j], 1);
}

// one workgroup: the slots, vertex order is elimination order
__global__ __launch_bounds__(EG_THREADS) void egrid_slots(EgridArgs A) {
  if (threadIdx.x != 0) return;
  const EgWs& W = A.G.W;
  EgridDev& D = *A.G.dev;
  if (D.bad) {
    D.state = EGRID_REFUSED;
    return;
  }
  int o = 0, nf = 0;
  for (int k = 0; k < A.L.n_kf; k++) {
    W.start[k] = o;
    o += W.cnt[k];
    if (!A.L.vertices[k].fixed && W.cnt[k] > 0) {
      W.kf_of_slot[nf] = k;
      W.slot[k] = nf++;
    } else {
      W.slot[k] = -1;
    }
  }
  W.start[A.L.n_kf] = o;
  D.n_free = nf;
  D.state = (nf == 0 || A.L.n_edges == 0) ? EGRID_IDLE : EGRID_READY;   // idle: optimize() has nothing to do
}

__global__ __launch_bounds__(EG_THREADS) void egrid_fill(EgridArgs A) {
  if (A.G.dev->state != EGRID_READY) return;
  const size_t e = egrid_gid();
  if (e < (size_t)A.L.n_edges) eg_list_fill(A.G.W, A.L.edges, (int)e);
}

__global__ __launch_bounds__(EG_THREADS) void egrid_sort(EgridArgs A) {
  if (A.G.dev->state != EGRID_READY) return;
  const size_t k = egrid_gid();
  if (k < (size_t)A.L.n_kf) eg_list_sort(A.G.W, (int)k);
}

__global__ __launch_bounds__(EG_THREADS) void egrid_first(EgridArgs A) {
  if (A.G.dev->state != EGRID_READY) return;
  const size_t r = egrid_gid();
  if (r < (size_t)A.G.dev->n_free) A.G.W.first[r] = eg_row_first(A.G.W, A.L.edges, (int)r);
}

// one workgroup: the row offsets; an envelope beyond what the workspace holds is refused.  Leaves the first control record
__global__ __launch_bounds__(EG_THREADS) void egrid_offsets(EgridArgs A) {
  if (threadIdx.x != 0) return;
  const EgWs& W = A.G.W;
  EgridDev& D = *A.G.dev;
  EgridControl& C = *A.G.control;
  if (D.state == EGRID_READY) {
    long long o = 0;
    for (int r = 0; r < D.n_free; r++) {
      W.row_off[r] = (int32_t)(o < 0x7fffffff ? o : 0x7fffffff);
      o += r - W.first[r] + 1;
    }
    D.total = o;
    if (o > A.L.env_cap) D.state = EGRID_REFUSED;
  }
  D.status = D.state == EGRID_REFUSED ? ORBFE_EG_REFUSED : ORBFE_EG_DONE;
  D.lambda = EG_LAMBDA_INIT;
  D.ni = 2.0;
  C.action = D.state == EGRID_READY ? EGRID_BUILD : EGRID_DONE;
  C.pop = 0;
  C.state = D.state;
  C.n_free = D.n_free;
  C.iterations = 0;
  C.trials = 0;
  C.total = D.total;
  C.lambda = 0.0;
  C.chi2 = 0.0;
}

// ---- linearise ----------------------------------------------------------------------------------------------------------------------
// SE3: a lane per edge.  Sim3: a lane per (edge, column) of the numeric Jacobian; the lane of column 0 also leaves the error and chi2
template <int D>
__global__ __launch_bounds__(EG_THREADS) void egrid_linearize(EgridArgs A) {
  const size_t t = egrid_gid();
  if constexpr (D == 7) {
    const size_t e = t / 7;
    const int d = (int)(t % 7);
    if (e >= (size_t)A.L.n_edges) return;
    const EgWs& W = A.G.W;
    const orbfe_eg_edge E = A.L.edges[e];
    eg_linearize_column(W.je + e * EG_EDGE_DOUBLES, W.meas[e], W.est[E.i], W.est[E.j], W.slot[E.i] >= 0, W.slot[E.j] >= 0, d);
    if (d == 0) A.G.chi[e] = eg_linearize_error<D>(W, E, (int)e);
  } else {
    if (t < (size_t)A.L.n_edges) A.G.chi[t] = eg_linearize<D>(A.G.W, A.L.edges[t], (int)t);
  }
}

template <int D>
__global__ __launch_bounds__(EG_THREADS) void egrid_b(EgridArgs A, int n) {
  const size_t t = egrid_gid();
  if (t < (size_t)n) A.G.W.b[t] = eg_b_entry<D>(A.G.W, (int)(t / D), (int)(t % D));
}

// ---- build --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EG_THREADS) void egrid_zero(EgridArgs A, size_t elements, int n) {
  const size_t stride = (size_t)gridDim.x * EG_THREADS;
  for (size_t t = egrid_gid(); t < elements; t += stride) A.G.W.env[t] = 0.0;
  const size_t t = egrid_gid();
  if (t < (size_t)n) A.G.W.y[t] = A.G.W.b[t];
}

template <int D>
__global__ __launch_bounds__(EG_THREADS) void egrid_build(EgridArgs A, int nf) {
  const size_t t = egrid_gid();
  if (t < (size_t)nf * (D * D))
    eg_h_entries<D>(A.G.W, A.L.edges, (int)(t / (D * D)), (int)((t % (D * D)) / D), (int)(t % D), A.G.dev->lambda);
}

// ---- factor: the blocks plan[begin .. begin + gridDim.x) of one level, a workgroup each -----------------------------------------------
template <int D>
__global__ __launch_bounds__(EG_THREADS) void egrid_factor_level(EgridArgs A, long long begin, int level) {
  __shared__ double tile[49];
  // fail[level & 1] is written by this launch and read by the next one only, so what a lane reads here is complete and uniform
  if (A.G.dev->fail[(level + 1) & 1]) {
    if (threadIdx.x == 0) A.G.dev->fail[level & 1] = 1;
    return;
  }
  const EgridBlock B = A.G.plan[begin + blockIdx.x];
  const EgRow<D> Rr(A.G.W, B.r);
  if (B.c < B.r) {
    const EgRow<D> Rc(A.G.W, B.c);
    eg_tile_offdiag<D>(tile, Rr, Rc, B.c);
    __syncthreads();
    if (threadIdx.x < D) eg_block_solve<D>(tile, Rr, Rc, B.c, threadIdx.x);
  } else {
    eg_tile_diag<D>(tile, Rr, B.r);
    __syncthreads();
    if (threadIdx.x == 0 && !eg_diag_cholesky<D>(tile, Rr, B.r)) A.G.dev->fail[level & 1] = 1;
  }
}

// ---- solve: ONE workgroup -------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(EG_THREADS) void egrid_solve(EgridArgs A, int nf) {
  __shared__ double v[8];
  if (egrid_failed(A)) return;
  eg_solve<D>(A.G.W, v, nf);
}

// ---- trial --------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(EG_THREADS) void egrid_update(EgridArgs A, int nf) {
  if (egrid_failed(A)) return;
  const size_t r = egrid_gid();
  if (r < (size_t)nf) eg_push_oplus<D>(A.G.W, (int)r);
}

template <int D>
__global__ __launch_bounds__(EG_THREADS) void egrid_chi(EgridArgs A) {
  if (egrid_failed(A)) return;
  const size_t e = egrid_gid();
  if (e < (size_t)A.L.n_edges) A.G.chi[e] = eg_edge_chi2<D>(A.G.W, A.L.edges[e], (int)e);
}

__global__ __launch_bounds__(EG_THREADS) void egrid_pop(EgridArgs A, int nf) {
  const size_t r = egrid_gid();
  if (r < (size_t)nf) eg_pop(A.G.W, (int)r);
}

// ---- control: ONE workgroup of EG_THREADS -------------------------------------------------------------------------------------------
// after_trial == 0: behind linearise -- the iteration's chi2.  after_trial == 1: behind a trial -- its chi2 and computeScale,
// lm_trial_scaled, and the loop rules of essential_graph_kernel
__global__ __launch_bounds__(EG_THREADS) void egrid_control(EgridArgs A, int n, int after_trial) {
  __shared__ double red[EG_WAVES * 2], tot[2];
  const int tid = threadIdx.x, n_e = A.L.n_edges;
  const EgWs& W = A.G.W;
  EgridDev& D = *A.G.dev;
  EgridControl& C = *A.G.control;
  const bool ok2 = !egrid_failed(A);
  const double lambda = D.lambda;
  __syncthreads();   // lane 0 rewrites both below
  if (!after_trial) {
    double v[2] = {0.0, 0.0};
    for (int e = tid; e < n_e; e += EG_THREADS) v[0] += A.G.chi[e];
    lm_reduce<1, 2, EG_WAVES>(v, red, tot, tid);
    if (tid == 0) {
      const double chi = tot[0];
      D.current_chi = chi;
      if (D.it == 0) D.chi2_first = chi;
      D.rho = 0.0;
      D.qmax = 0;
      D.fail[0] = D.fail[1] = 0;
      C.action = EGRID_TRIAL;
      C.pop = 0;
      C.lambda = lambda;
      C.chi2 = chi;
    }
    return;
  }
  double temp_chi = 0.0, scale = 0.0;
  if (ok2) {   // uniform
    double u[2] = {0.0, 0.0};
    for (int t = tid; t < n; t += EG_THREADS) u[1] += eg_scale_term(W, t, lambda);   // computeScale
    for (int e = tid; e < n_e; e += EG_THREADS) u[0] += A.G.chi[e];
    lm_reduce<2, 2, EG_WAVES>(u, red, tot, tid);
    temp_chi = tot[0];
    scale = tot[1];
  }
  if (tid != 0) return;
  LmState lm;
  lm.lambda = lambda;
  lm.ni = D.ni;
  double rho = 0.0, current_chi = D.current_chi;
  int qmax = D.qmax, pop = 0;
  bool broke = false;
  if (!ok2) D.status = ORBFE_EG_FACTOR_FAILED;
  D.trials++;
  if (lm_trial_scaled(lm, ok2, current_chi, temp_chi, scale, &rho)) {
    current_chi = temp_chi;
  } else {
    pop = ok2 ? 1 : 0;
    if (!isfinite(lm.lambda)) broke = true;
  }
  if (!broke) qmax++;
  int action = EGRID_TRIAL;
  if (broke || !(rho < 0 && qmax < 10)) {
    D.iterations++;
    D.it++;
    action = (qmax == 10 || rho == 0 || !isfinite(lm.lambda) || D.it >= EG_ITERATIONS) ? EGRID_DONE : EGRID_BUILD;
  }
  D.lambda = lm.lambda;
  D.ni = lm.ni;
  D.rho = rho;
  D.qmax = qmax;
  D.current_chi = current_chi;
  D.fail[0] = D.fail[1] = 0;
  C.action = action;
  C.pop = pop;
  C.iterations = D.iterations;
  C.trials = D.trials;
  C.lambda = lm.lambda;
  C.chi2 = current_chi;
}

// ---- write-back ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EG_THREADS) void egrid_write(EgridArgs A) {
  const bool se3 = (A.L.flags & ORBFE_EG_FIX_SCALE) != 0;
  const EgridDev& D = *A.G.dev;
  const size_t k = egrid_gid();
  if (k < (size_t)A.L.n_kf) {
    if (D.state == EGRID_READY)
      eg_write_vertex(A.G.W, A.L.vertices, (int)k, se3, A.L.sim3_out, A.L.poses_out);
    else
      eg_write_through(A.L.vertices, (int)k, se3, A.L.sim3_out, A.L.poses_out);
  }
  if (k == 0) {
    orbfe_eg_result res = eg_result_refused(A.L.n_edges);
    res.status = D.status;
    res.n_free = D.n_free;
    res.envelope_blocks = (int32_t)(D.total < 0x7fffffff ? D.total : 0x7fffffff);
    if (D.state == EGRID_READY) {
      res.iterations = D.iterations;
      res.trials = D.trials;
      res.chi2_first = D.chi2_first;
      res.chi2_last = D.current_chi;
      res.lambda = D.lambda;
    }
    *A.L.result = res;
  }
}

// ---- the host loop ------------------------------------------------------------------------------------------------------------------
static inline dim3 grid_for(size_t items) { return dim3((unsigned)std::max<size_t>(1, (items + EG_THREADS - 1) / EG_THREADS)); }

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

template <int D>
static hipError_t run(const EgridArgs& A, EgridControl* pinned, hipStream_t s, float* phase_ms, int* levels_out) {
  const EgridLaunch& L = A.L;
  const EgridWs& G = A.G;
  const dim3 one(1), wg(EG_THREADS), g_kf = grid_for((size_t)L.n_kf), g_e = grid_for((size_t)L.n_edges);
  Phases ph(phase_ms, s);
  hipError_t e;
  auto read_control = [&]() -> hipError_t {
    ph.begin();
    hipError_t r = hipMemcpyAsync(pinned, G.control, sizeof(EgridControl), hipMemcpyDeviceToHost, s);
    if (r == hipSuccess) r = hipStreamSynchronize(s);
    ph.end(EGRID_PH_CONTROL);
    return r;
  };

  // prepare, once per call
  ph.begin();
  if ((e = hipMemsetAsync(G.dev, 0, sizeof(EgridDev), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(egrid_check, grid_for(std::max((size_t)L.n_kf, (size_t)L.n_edges)), wg, 0, s, A);
  hipLaunchKernelGGL(egrid_measure, g_e, wg, 0, s, A);
  hipLaunchKernelGGL(egrid_slots, one, wg, 0, s, A);
  hipLaunchKernelGGL(egrid_fill, g_e, wg, 0, s, A);
  hipLaunchKernelGGL(egrid_sort, g_kf, wg, 0, s, A);
  hipLaunchKernelGGL(egrid_first, g_kf, wg, 0, s, A);   // n_free <= n_kf
  hipLaunchKernelGGL(egrid_offsets, one, wg, 0, s, A);
  ph.end(EGRID_PH_PREPARE);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = read_control()) != hipSuccess) return e;

  if (pinned->state == EGRID_READY) {
    const int nf = pinned->n_free, n = nf * D;
    const size_t elements = (size_t)pinned->total * (D * D);

    // the level plan, once per call, on the host: first[] down, the blocks sorted by level up
    ph.begin();
    std::vector<int32_t> first((size_t)nf);
    if ((e = hipMemcpyAsync(first.data(), G.W.first, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    std::vector<int64_t> level_start;
    std::vector<EgridBlock> blocks;
    const int levels = eg_level_plan(first.data(), nf, level_start, &blocks, nullptr);
    if ((int64_t)blocks.size() != (int64_t)pinned->total || levels > eg_plan_level_bound(nf)) return hipErrorAssert;   // the two sides drifted apart
    if ((e = hipMemcpyAsync(G.plan, blocks.data(), blocks.size() * sizeof(EgridBlock), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    ph.end(EGRID_PH_PLAN);
    if (levels_out) *levels_out = levels;

    // at most 20 iterations x 10 trials, one read of the control record each
    const int max_trials = EG_ITERATIONS * 10;
    const dim3 g_zero = dim3(std::min<unsigned>(grid_for(std::max(elements, (size_t)n)).x, 1u << 20));
    int action = EGRID_BUILD;
    for (int trial = 0; trial < max_trials && action != EGRID_DONE; trial++) {
      if (action == EGRID_BUILD) {
        ph.begin();
        hipLaunchKernelGGL(egrid_linearize<D>, D == 7 ? grid_for((size_t)L.n_edges * 7) : g_e, wg, 0, s, A);
        hipLaunchKernelGGL(egrid_b<D>, grid_for((size_t)n), wg, 0, s, A, n);
        hipLaunchKernelGGL(egrid_control, one, wg, 0, s, A, n, 0);
        ph.end(EGRID_PH_LINEARIZE);
      }
      ph.begin();
      hipLaunchKernelGGL(egrid_zero, g_zero, wg, 0, s, A, elements, n);
      hipLaunchKernelGGL(egrid_build<D>, grid_for((size_t)nf * (D * D)), wg, 0, s, A, nf);
      ph.end(EGRID_PH_BUILD);
      ph.begin();
      for (int l = 0; l < levels; l++)   // levels <= 2 n_free + 1; no level is empty
        hipLaunchKernelGGL(egrid_factor_level<D>, dim3((unsigned)(level_start[l + 1] - level_start[l])), wg, 0, s, A,
                           (long long)level_start[l], l);
      ph.end(EGRID_PH_FACTOR);
      ph.begin();
      hipLaunchKernelGGL(egrid_solve<D>, one, wg, 0, s, A, nf);
      ph.end(EGRID_PH_SOLVE);
      ph.begin();
      hipLaunchKernelGGL(egrid_update<D>, grid_for((size_t)nf), wg, 0, s, A, nf);
      hipLaunchKernelGGL(egrid_chi<D>, g_e, wg, 0, s, A);
      hipLaunchKernelGGL(egrid_control, one, wg, 0, s, A, n, 1);
      ph.end(EGRID_PH_UPDATE);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = read_control()) != hipSuccess) return e;
      action = pinned->action;
      if (pinned->pop) hipLaunchKernelGGL(egrid_pop, grid_for((size_t)nf), wg, 0, s, A, nf);
    }
  }
  hipLaunchKernelGGL(egrid_write, g_kf, wg, 0, s, A);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipStreamSynchronize(s);
}

hipError_t orbfe_run_egrid(const EgridLaunch& L, const EgridWs& G, EgridControl* pinned, hipStream_t s, float* phase_ms, int* levels) {
  EgridArgs A;
  A.L = L;
  A.G = G;
  return (L.flags & ORBFE_EG_FIX_SCALE) ? run<6>(A, pinned, s, phase_ms, levels) : run<7>(A, pinned, s, phase_ms, levels);
}
