// egraph_grid_internal.h -- what egraph_grid_kernels.hip and egraph_grid.cpp share: the workspace of ONE graph of
// Optimizer::OptimizeEssentialGraph that the whole grid works on, the level plan of its factorisation, the records the control kernel
// leaves for the host loop, and the launch interface.  The arithmetic is egraph_internal.h's and the per-item steps are
// egraph_steps.h's; this header adds no formula of its own.
//
// The level plan.  Block (r, c) of the up-looking block L L^T needs row r's blocks before c and the whole of row c, so
//   level(r, c) = 1 + max(level(r, c - 1) if c > first[r], level(c, c))   for c < r
//   level(r, r) = 1 + level(r, r - 1), or 1 for a row that holds its diagonal block only
// With g(c) = level(c, c) - c this is level(r, c) = c + 1 + max g over first[r] .. c: a prefix maximum along the row, strictly
// increasing in c, so a row has at most one block per level.  By induction level(c, c) <= 2 c + 1, so there are at most 2 n_free
// levels; eg_plan_level_bound states 2 n_free + 1, and that bounds the host's launch loop.  The structure does not change between
// trials: the plan is computed once per call, ON THE HOST, from first[] (one download of n_free ints), and uploaded as the list of
// blocks sorted by level.
#pragma once
#include <vector>

#include "egraph_internal.h"

enum { EGRID_TRIAL = 0, EGRID_BUILD = 1, EGRID_DONE = 2 };      // EgridControl.action: what the host enqueues next
enum { EGRID_REFUSED = 0, EGRID_IDLE = 1, EGRID_READY = 2 };    // EgridDev.state

struct EgridDev {     // the graph's state, in HBM; written by one-workgroup kernels only (bad, fail: the same value by many lanes)
  int state, bad, n_free, reserved0;
  int fail[2];       // a pivot that was not > 0 at a level of this parity, or handed on from the level before
  int it, qmax, iterations, trials;
  int status, reserved;
  long long total;   // blocks of the row envelope
  double lambda, ni, current_chi, chi2_first, rho;
};

struct EgridControl {  // what the host loop reads once per trial
  int action, pop, state, n_free, iterations, trials;
  long long total;
  double lambda, chi2;
};

struct EgridBlock {   // one block of the envelope in the level plan
  int32_t r, c;
};

struct EgridWs {      // carved over the caller's workspace for kf_cap vertices, edge_cap edges and env_cap envelope blocks
  EgWs W;             // egraph_internal.h's arrays
  double* chi;        // [edge_cap] the chi2 of every edge, summed by the control kernel in the one workgroup's order
  EgridBlock* plan;   // [env_cap] the blocks sorted by level
  EgridDev* dev;
  EgridControl* control;
};

// the part that does not depend on env_cap lies in front, so a workspace states how many blocks it holds
__host__ __device__ inline size_t egrid_fixed_bytes(int kf_cap, int edge_cap) {
  return eg_ws_bytes(kf_cap, edge_cap, 0) + eg_align((size_t)edge_cap * 8) + eg_align(sizeof(EgridDev)) + eg_align(sizeof(EgridControl));
}
__host__ __device__ inline size_t egrid_ws_bytes(int kf_cap, int edge_cap, int64_t env_cap) {
  return egrid_fixed_bytes(kf_cap, edge_cap) + eg_align((size_t)env_cap * sizeof(EgridBlock)) + eg_align((size_t)env_cap * 49 * 8);
}
// the largest env_cap a workspace of `bytes` holds (bytes >= egrid_fixed_bytes)
inline int64_t egrid_env_cap_of(int kf_cap, int edge_cap, size_t bytes, int64_t limit) {
  int64_t v = (int64_t)((bytes - egrid_fixed_bytes(kf_cap, edge_cap)) / (49 * 8 + sizeof(EgridBlock)));
  if (v > limit) v = limit;
  while (v > 0 && egrid_ws_bytes(kf_cap, edge_cap, v) > bytes) v--;
  return v;
}
inline void egrid_ws_carve(uint8_t* base, int kf_cap, int edge_cap, int64_t env_cap, EgridWs& G) {
  eg_ws_carve(base, kf_cap, edge_cap, 0, G.W);   // env: zero bytes here, placed below
  uint8_t* p = base + eg_ws_bytes(kf_cap, edge_cap, 0);
  G.chi = (double*)p; p += eg_align((size_t)edge_cap * 8);
  G.dev = (EgridDev*)p; p += eg_align(sizeof(EgridDev));
  G.control = (EgridControl*)p; p += eg_align(sizeof(EgridControl));
  G.plan = (EgridBlock*)p; p += eg_align((size_t)env_cap * sizeof(EgridBlock));
  G.W.env = (double*)p;
}

inline int64_t eg_plan_level_bound(int n_free) { return 2 * (int64_t)n_free + 1; }

// The level plan from first[n_free].  level_start[l] .. level_start[l + 1]: the blocks of level l + 1 in `blocks` (rows ascending);
// block_level (optional): the level of every block in envelope order (row by row, columns ascending).  Returns the level count.
inline int eg_level_plan(const int32_t* first, int n_free, std::vector<int64_t>& level_start, std::vector<EgridBlock>* blocks,
                         int32_t* block_level) {
  std::vector<int32_t> g(n_free);   // level(c, c) - c
  std::vector<int64_t> count;
  int levels = 0;
  for (int pass = 0; pass < 2; pass++) {   // count, then place
    std::vector<int64_t> at;
    if (pass == 1) {
      level_start.assign((size_t)levels + 1, 0);
      for (int l = 0; l < levels; l++) level_start[l + 1] = level_start[l] + count[l];
      at.assign(level_start.begin(), level_start.end() - 1);
      if (blocks) blocks->resize((size_t)level_start[levels]);
    }
    int64_t o = 0;
    for (int r = 0; r < n_free; r++) {
      int32_t m = INT32_MIN, lv = 0;
      for (int c = first[r]; c < r; c++, o++) {
        m = g[c] > m ? g[c] : m;
        lv = c + 1 + m;
        if (pass == 0) {
          if ((size_t)lv > count.size()) count.resize(lv, 0);
          count[lv - 1]++;
          if (block_level) block_level[o] = lv;
        } else if (blocks) {
          (*blocks)[(size_t)at[lv - 1]++] = EgridBlock{r, c};
        }
      }
      lv = lv + 1;   // the diagonal block
      g[r] = lv - r;
      if (pass == 0) {
        if ((size_t)lv > count.size()) count.resize(lv, 0);
        count[lv - 1]++;
        if (block_level) block_level[o] = lv;
      } else if (blocks) {
        (*blocks)[(size_t)at[lv - 1]++] = EgridBlock{r, r};
      }
      o++;
    }
    if (pass == 0) levels = (int)count.size();
  }
  return levels;
}

// egraph.cpp: the validation both forms share.  Everything the host can see of one graph on host arrays: counts, flags, null arrays,
// edges, records, derived scales; *env: the blocks of its row envelope.  ORBFE_OK or ORBFE_ERR_INVALID with the error text set
int eg_validate_host_graph(const char* who, const orbfe_eg_vertex* vertices, int n_kf, const orbfe_eg_edge* edges, int n_edges, int flags,
                           const void* sim3_out, const void* poses_out, const void* result, int64_t* env);
bool eg_counts_ok(const char* who, int n_kf, int n_edges);

struct EgridLaunch {   // the arguments of orbfe_essential_graph_grid_device, all in HBM
  const orbfe_eg_vertex* vertices;
  const orbfe_eg_edge* edges;
  int n_kf, n_edges, flags;
  int64_t env_cap;
  orbfe_eg_sim3* sim3_out;
  float* poses_out;
  orbfe_eg_result* result;
};

// egraph_grid_kernels.hip: the whole call on `s`; synchronous.  pinned: an EgridControl in pinned host memory.  phase_ms: null, or
// EGRID_PHASES sums of stream-event times (prepare, the host's level plan and its upload, linearise, build, factorisation, solves,
// update / chi2 / control kernel, control read-back); levels: null, or where the level count of the plan goes
enum { EGRID_PH_PREPARE, EGRID_PH_PLAN, EGRID_PH_LINEARIZE, EGRID_PH_BUILD, EGRID_PH_FACTOR, EGRID_PH_SOLVE, EGRID_PH_UPDATE,
       EGRID_PH_CONTROL, EGRID_PHASES };
hipError_t orbfe_run_egrid(const EgridLaunch& L, const EgridWs& G, EgridControl* pinned, hipStream_t s, float* phase_ms, int* levels);
