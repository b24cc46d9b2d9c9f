// egraph_grid.cpp -- C ABI of the essential-graph optimisation of one graph across the device (include/orbfe.h:
// orbfe_essential_graph_grid, orbfe_essential_graph_grid_workspace_bytes, orbfe_essential_graph_grid_device,
// orbfe_debug_egrid_phases, orbfe_debug_egrid_level_plan).  The entry points validate against the ORBFE_EGRID_MAX_* limits before any
// device is looked for -- the host form with egraph.cpp's validation --, stage (HostCall) as egraph.cpp does for the one-workgroup form,
// carve the workspace, keep the pinned control record for the length of the call and hand the graph to the host loop of
// egraph_grid_kernels.hip.  No CPU fallback: without a device both forms are an error.
#include <string.h>

#include <vector>

#include "egraph_grid_internal.h"
#include "host_internal.h"

static_assert(ORBFE_EGRID_MAX_KEYFRAMES == ORBFE_EG_MAX_KEYFRAMES && ORBFE_EGRID_MAX_EDGES == ORBFE_EG_MAX_EDGES,
              "eg_counts_ok states the counts of both forms");

static const char* WHO = "essential graph grid";

static bool env_ok(const char* who, int64_t env) {
  if (env < 0 || env > ORBFE_EGRID_MAX_ENVELOPE_BLOCKS) {
    orbfe_set_error("%s: the row envelope has %lld blocks (0 .. %d): list the keyframes by ascending mnId", who, (long long)env,
                    ORBFE_EGRID_MAX_ENVELOPE_BLOCKS);
    return false;
  }
  return true;
}

extern "C" int orbfe_essential_graph_grid_workspace_bytes(int kf_cap, int edge_cap, int64_t env_cap, size_t* bytes) {
  const char* who = "essential graph grid workspace bytes";
  if (!bytes) {
    orbfe_set_error("%s: bytes is required", who);
    return ORBFE_ERR_INVALID;
  }
  if (!eg_counts_ok(who, kf_cap, edge_cap) || !env_ok(who, env_cap)) return ORBFE_ERR_INVALID;
  *bytes = egrid_ws_bytes(kf_cap, edge_cap, env_cap);
  return ORBFE_OK;
}

extern "C" int orbfe_debug_egrid_level_plan(const int32_t* first, int n_free, int32_t* block_level, int32_t* n_levels) {
  const char* who = "essential graph grid level plan";
  if (n_free < 0 || n_free > ORBFE_EGRID_MAX_KEYFRAMES || !n_levels || (n_free > 0 && (!first || !block_level))) {
    orbfe_set_error("%s: n_free %d (0 .. %d); first, block_level and n_levels are required", who, n_free, ORBFE_EGRID_MAX_KEYFRAMES);
    return ORBFE_ERR_INVALID;
  }
  int64_t total = 0;
  for (int r = 0; r < n_free; r++) {
    if (first[r] < 0 || first[r] > r) {
      orbfe_set_error("%s: first[%d] = %d (0 .. %d)", who, r, first[r], r);
      return ORBFE_ERR_INVALID;
    }
    total += r - first[r] + 1;
  }
  if (!env_ok(who, total)) return ORBFE_ERR_INVALID;
  std::vector<int64_t> level_start;
  *n_levels = eg_level_plan(first, n_free, level_start, nullptr, block_level);
  return ORBFE_OK;
}

// the control record's pinned mirror, for the length of one call
struct PinnedControl {
  EgridControl* p = nullptr;
  ~PinnedControl() {
    if (p) (void)hipHostFree(p);
  }
};

// orbfe_debug_egrid_phases: the calling thread's switch, its sums of stream-event times per phase and the last call's level count
static thread_local bool t_timing = false;
static thread_local float t_phase_ms[EGRID_PHASES + 1];

extern "C" int orbfe_debug_egrid_phases(int enable, float* ms) {
  if (ms) memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  memset(t_phase_ms, 0, sizeof(t_phase_ms));
  t_timing = enable != 0;
  return ORBFE_OK;
}

static int run(const EgridLaunch& L, void* d_workspace, hipStream_t stream) {
  PinnedControl pc;
  int rc;
  if ((rc = hip_status("essential graph grid: control record", hipHostMalloc((void**)&pc.p, sizeof(EgridControl), hipHostMallocDefault))))
    return rc;
  EgridWs G;
  egrid_ws_carve((uint8_t*)d_workspace, L.n_kf, L.n_edges, L.env_cap, G);
  int levels = 0;
  rc = hip_status("essential graph grid: launch", orbfe_run_egrid(L, G, pc.p, stream, t_timing ? t_phase_ms : nullptr, &levels));
  if (t_timing) t_phase_ms[EGRID_PHASES] = (float)levels;
  return rc;
}

extern "C" int orbfe_essential_graph_grid_device(const orbfe_eg_vertex* d_vertices, int n_kf, const orbfe_eg_edge* d_edges, int n_edges,
                                                 int flags, orbfe_eg_sim3* d_sim3_out, float* d_poses_out, orbfe_eg_result* d_result,
                                                 void* d_workspace, size_t workspace_bytes, void* stream) {
  const char* who = "essential graph grid device";
  if (!eg_counts_ok(who, n_kf, n_edges)) return ORBFE_ERR_INVALID;
  if (flags & ~ORBFE_EG_FIX_SCALE) {
    orbfe_set_error("%s: flags %d", who, flags);
    return ORBFE_ERR_INVALID;
  }
  if (!d_result || (n_kf > 0 && (!d_vertices || !d_sim3_out || !d_poses_out)) || (n_edges > 0 && !d_edges)) {
    orbfe_set_error("%s: every pointer is required (the arrays of a count of 0 may be null)", who);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_vertices & 7) || ((uintptr_t)d_edges & 3) || ((uintptr_t)d_sim3_out & 7) || ((uintptr_t)d_poses_out & 3) ||
      ((uintptr_t)d_result & 7)) {
    orbfe_set_error("%s: vertices, sim3_out and result must be 8-byte aligned, the other records 4-byte", who);
    return ORBFE_ERR_INVALID;
  }
  const size_t need = egrid_ws_bytes(n_kf, n_edges, 0);
  if (!d_workspace || workspace_bytes < need || ((uintptr_t)d_workspace & 255)) {
    orbfe_set_error("%s: the workspace needs at least %zu bytes at a 256-byte boundary (%zu given)", who, need, workspace_bytes);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  EgridLaunch L;
  memset(&L, 0, sizeof(L));
  L.vertices = d_vertices; L.edges = d_edges; L.n_kf = n_kf; L.n_edges = n_edges; L.flags = flags;
  L.env_cap = egrid_env_cap_of(n_kf, n_edges, workspace_bytes, ORBFE_EGRID_MAX_ENVELOPE_BLOCKS);   // what the workspace holds
  L.sim3_out = d_sim3_out; L.poses_out = d_poses_out; L.result = d_result;
  return run(L, d_workspace, (hipStream_t)stream);
}

extern "C" int orbfe_essential_graph_grid(const orbfe_eg_vertex* vertices, int n_kf, const orbfe_eg_edge* edges, int n_edges, int flags,
                                          orbfe_eg_sim3* sim3_out, float* poses_out, orbfe_eg_result* result) {
  int64_t env = 0;
  int rc;
  if ((rc = eg_validate_host_graph(WHO, vertices, n_kf, edges, n_edges, flags, sim3_out, poses_out, result, &env))) return rc;
  if (!env_ok(WHO, env)) return ORBFE_ERR_INVALID;
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;

  // the workspace is an allocation of its own; its guard is declared before the call, so it is freed after the call has drained
  struct Workspace {
    void* p = nullptr;
    ~Workspace() {
      if (p) (void)hipFree(p);
    }
  } ws;
  HostCall c(WHO);
  const size_t o_v = c.in((size_t)n_kf * sizeof(orbfe_eg_vertex)), o_e = c.in((size_t)n_edges * sizeof(orbfe_eg_edge));
  const size_t o_res = c.out(sizeof(orbfe_eg_result)), o_s = c.out((size_t)n_kf * sizeof(orbfe_eg_sim3)), o_p = c.out((size_t)n_kf * 48);
  if ((rc = c.open())) return rc;
  if ((rc = hip_status("essential graph grid: workspace", hipMalloc(&ws.p, egrid_ws_bytes(n_kf, n_edges, env))))) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  if (n_kf) memcpy(h + o_v, vertices, (size_t)n_kf * sizeof(orbfe_eg_vertex));
  if (n_edges) memcpy(h + o_e, edges, (size_t)n_edges * sizeof(orbfe_eg_edge));
  if (c.in_end() && (rc = c.upload())) return rc;   // a graph without a vertex has nothing to upload
  EgridLaunch L;
  memset(&L, 0, sizeof(L));
  L.vertices = (const orbfe_eg_vertex*)(d + o_v); L.edges = (const orbfe_eg_edge*)(d + o_e); L.n_kf = n_kf; L.n_edges = n_edges;
  L.flags = flags; L.env_cap = env; L.sim3_out = (orbfe_eg_sim3*)(d + o_s); L.poses_out = (float*)(d + o_p);
  L.result = (orbfe_eg_result*)(d + o_res);
  if ((rc = run(L, ws.p, c.stream))) return rc;
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(result, h + o_res, sizeof(orbfe_eg_result));
  if (n_kf) memcpy(sim3_out, h + o_s, (size_t)n_kf * sizeof(orbfe_eg_sim3));
  if (n_kf) memcpy(poses_out, h + o_p, (size_t)n_kf * 48);
  if (result->status == ORBFE_EG_REFUSED) {   // the kernels' limits are the host's: unreachable unless the two drift apart
    orbfe_set_error("%s: refused on the device", WHO);
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
}
