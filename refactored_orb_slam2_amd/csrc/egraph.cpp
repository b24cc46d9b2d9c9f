// egraph.cpp -- C ABI of Optimizer::OptimizeEssentialGraph and of the map correction behind it (include/orbfe.h:
// orbfe_essential_graph, orbfe_essential_graph_batch_device, orbfe_essential_graph_envelope_blocks,
// orbfe_essential_graph_workspace_bytes, orbfe_sim3_correct_points, orbfe_sim3_correct_points_device).  The entry points validate,
// stage and launch egraph_kernels.hip.  No CPU fallback: without a device the compute forms are an error.
#include <math.h>
#include <string.h>

#include <vector>

#include "egraph_grid_internal.h"
#include "host_internal.h"

static const char* WHO = "essential graph";

bool eg_counts_ok(const char* who, int n_kf, int n_edges) {
  if (n_kf < 0 || n_kf > ORBFE_EG_MAX_KEYFRAMES || n_edges < 0 || n_edges > ORBFE_EG_MAX_EDGES) {
    orbfe_set_error("%s: n_kf %d (0 .. %d), n_edges %d (0 .. %d)", who, n_kf, ORBFE_EG_MAX_KEYFRAMES, n_edges, ORBFE_EG_MAX_EDGES);
    return false;
  }
  return true;
}

static bool edges_ok(const char* who, const orbfe_eg_edge* edges, int n_edges, int n_kf) {
  for (int e = 0; e < n_edges; e++) {
    const orbfe_eg_edge& E = edges[e];
    if (E.i < 0 || E.i >= n_kf || E.j < 0 || E.j >= n_kf || E.i == E.j || E.kind > ORBFE_EG_LOOP_CONNECTION) {
      orbfe_set_error("%s: edge %d: i %d, j %d (0 .. %d, different), kind %u (0, 1)", who, e, E.i, E.j, n_kf - 1, E.kind);
      return false;
    }
  }
  return true;
}

// the row envelope in vertex order: one diagonal block per vertex in the system, and one per free vertex from the earliest neighbour on
static int64_t envelope(int n_kf, const uint8_t* fixed, const orbfe_eg_edge* edges, int n_edges) {
  std::vector<int32_t> slot(n_kf, -1), first;
  std::vector<uint8_t> has(n_kf, 0);
  for (int e = 0; e < n_edges; e++) has[edges[e].i] = has[edges[e].j] = 1;
  int nf = 0;
  for (int k = 0; k < n_kf; k++)
    if (has[k] && !(fixed && fixed[k])) slot[k] = nf++;
  first.resize(nf);
  for (int r = 0; r < nf; r++) first[r] = r;
  for (int e = 0; e < n_edges; e++) {
    const int a = slot[edges[e].i], b = slot[edges[e].j];
    if (a < 0 || b < 0) continue;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (lo < first[hi]) first[hi] = lo;
  }
  int64_t total = 0;
  for (int r = 0; r < nf; r++) total += r - first[r] + 1;
  return total;
}

extern "C" int orbfe_essential_graph_envelope_blocks(int n_kf, const uint8_t* fixed, const orbfe_eg_edge* edges, int n_edges, int64_t* blocks) {
  const char* who = "essential graph envelope blocks";
  if (!blocks || (n_edges > 0 && !edges)) {
    orbfe_set_error("%s: blocks and, with n_edges > 0, edges are required", who);
    return ORBFE_ERR_INVALID;
  }
  if (!eg_counts_ok(who, n_kf, n_edges) || !edges_ok(who, edges, n_edges, n_kf)) return ORBFE_ERR_INVALID;
  *blocks = envelope(n_kf, fixed, edges, n_edges);
  return ORBFE_OK;
}

static bool caps_ok(const char* who, int P, int kf_cap, int edge_cap, int env_cap) {
  if (P < 0 || P > ORBFE_EG_MAX_PROBLEMS || kf_cap < 0 || kf_cap > ORBFE_EG_MAX_KEYFRAMES || edge_cap < 0 || edge_cap > ORBFE_EG_MAX_EDGES ||
      env_cap < 0 || env_cap > ORBFE_EG_MAX_ENVELOPE_BLOCKS) {
    orbfe_set_error("%s: P %d (0 .. %d), kf_cap %d (0 .. %d), edge_cap %d (0 .. %d), env_cap %d (0 .. %d)", who, P, ORBFE_EG_MAX_PROBLEMS,
                    kf_cap, ORBFE_EG_MAX_KEYFRAMES, edge_cap, ORBFE_EG_MAX_EDGES, env_cap, ORBFE_EG_MAX_ENVELOPE_BLOCKS);
    return false;
  }
  return true;
}

extern "C" int orbfe_essential_graph_workspace_bytes(int P, int kf_cap, int edge_cap, int env_cap, size_t* bytes) {
  if (!bytes) {
    orbfe_set_error("essential graph workspace bytes: bytes is required");
    return ORBFE_ERR_INVALID;
  }
  if (!caps_ok("essential graph workspace bytes", P, kf_cap, edge_cap, env_cap)) return ORBFE_ERR_INVALID;
  *bytes = (size_t)P * eg_ws_bytes(kf_cap, edge_cap, env_cap);
  return ORBFE_OK;
}

extern "C" int orbfe_essential_graph_batch_device(int P, const orbfe_eg_problem* d_problems, const orbfe_eg_vertex* d_vertices,
                                                  const orbfe_eg_edge* d_edges, int kf_cap, int edge_cap, int env_cap, int flags,
                                                  orbfe_eg_sim3* d_sim3_out, float* d_poses_out, orbfe_eg_result* d_result,
                                                  void* d_workspace, size_t workspace_bytes, void* stream) {
  const char* who = "essential graph batch";
  if (!caps_ok(who, P, kf_cap, edge_cap, env_cap)) return ORBFE_ERR_INVALID;
  if (flags & ~ORBFE_EG_FIX_SCALE) {
    orbfe_set_error("%s: flags %d", who, flags);
    return ORBFE_ERR_INVALID;
  }
  if (!d_problems || !d_result || (kf_cap > 0 && (!d_vertices || !d_sim3_out || !d_poses_out)) || (edge_cap > 0 && !d_edges)) {
    orbfe_set_error("%s: every pointer is required (the arrays of a cap of 0 may be null)", who);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_problems & 3) || ((uintptr_t)d_vertices & 7) || ((uintptr_t)d_edges & 3) || ((uintptr_t)d_sim3_out & 7) ||
      ((uintptr_t)d_poses_out & 3) || ((uintptr_t)d_result & 7)) {
    orbfe_set_error("%s: vertices, sim3_out and result must be 8-byte aligned, the other records 4-byte", who);
    return ORBFE_ERR_INVALID;
  }
  const size_t need = (size_t)P * eg_ws_bytes(kf_cap, edge_cap, env_cap);
  if (need > 0 && (!d_workspace || workspace_bytes < need || ((uintptr_t)d_workspace & 255))) {
    orbfe_set_error("%s: the workspace needs %zu bytes at a 256-byte boundary (%zu given)", who, need, workspace_bytes);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (P == 0) return ORBFE_OK;
  EgLaunch L;
  memset(&L, 0, sizeof(L));
  L.problems = d_problems; L.vertices = d_vertices; L.edges = d_edges; L.kf_cap = kf_cap; L.edge_cap = edge_cap; L.env_cap = env_cap;
  L.flags = flags; L.sim3_out = d_sim3_out; L.poses_out = d_poses_out; L.result = d_result; L.workspace = (uint8_t*)d_workspace;
  orbfe_launch_essential_graph(L, P, (hipStream_t)stream);
  return hip_status("essential graph batch: kernel launch failed", hipGetLastError());
}

// what both host forms of one graph check before a device is looked for (egraph_grid_internal.h)
int eg_validate_host_graph(const char* who, const orbfe_eg_vertex* vertices, int n_kf, const orbfe_eg_edge* edges, int n_edges, int flags,
                           const void* sim3_out, const void* poses_out, const void* result, int64_t* env) {
  if (!result) {
    orbfe_set_error("%s: result is required", who);
    return ORBFE_ERR_INVALID;
  }
  if (!eg_counts_ok(who, n_kf, n_edges)) return ORBFE_ERR_INVALID;
  if (flags & ~ORBFE_EG_FIX_SCALE) {
    orbfe_set_error("%s: flags %d", who, flags);
    return ORBFE_ERR_INVALID;
  }
  if ((n_kf > 0 && (!vertices || !sim3_out || !poses_out)) || (n_edges > 0 && !edges)) {
    orbfe_set_error("%s: the arrays of a count > 0 are required", who);
    return ORBFE_ERR_INVALID;
  }
  if (!edges_ok(who, edges, n_edges, n_kf)) return ORBFE_ERR_INVALID;
  const bool se3 = (flags & ORBFE_EG_FIX_SCALE) != 0;
  std::vector<uint8_t> fixed(n_kf);
  for (int k = 0; k < n_kf; k++) {
    const orbfe_eg_vertex& v = vertices[k];
    if (!eg_record_ok(v.Scw) || !eg_record_ok(v.Snc)) {
      orbfe_set_error("%s: vertex %d: a record must be finite with s > 0 and a quaternion of non-zero norm", who, k);
      return ORBFE_ERR_INVALID;
    }
    if (se3 && (!eg_unit_scale(v.Scw.s) || !eg_unit_scale(v.Snc.s))) {
      orbfe_set_error("%s: vertex %d: scales %.17g, %.17g with a fixed scale (|s - 1| <= 1e-3)", who, k, v.Scw.s, v.Snc.s);
      return ORBFE_ERR_INVALID;
    }
    fixed[k] = v.fixed ? 1 : 0;
  }
  if (se3)
    for (int e = 0; e < n_edges; e++) {
      const orbfe_eg_edge& E = edges[e];
      const bool loop = E.kind == ORBFE_EG_LOOP_CONNECTION;
      const double s = eg_measurement_scale(loop ? vertices[E.i].Scw.s : vertices[E.i].Snc.s, loop ? vertices[E.j].Scw.s : vertices[E.j].Snc.s);
      if (!eg_unit_scale(s)) {
        orbfe_set_error("%s: edge %d: its measurement has scale %.17g with a fixed scale (|s - 1| <= 1e-3)", who, e, s);
        return ORBFE_ERR_INVALID;
      }
    }
  *env = envelope(n_kf, fixed.data(), edges, n_edges);
  return ORBFE_OK;
}

extern "C" int orbfe_essential_graph(const orbfe_eg_vertex* vertices, int n_kf, const orbfe_eg_edge* edges, int n_edges, int flags,
                                     orbfe_eg_sim3* sim3_out, float* poses_out, orbfe_eg_result* result) {
  int64_t env = 0;
  int rc;
  if ((rc = eg_validate_host_graph(WHO, vertices, n_kf, edges, n_edges, flags, sim3_out, poses_out, result, &env))) return rc;
  if (env > ORBFE_EG_MAX_ENVELOPE_BLOCKS) {
    orbfe_set_error("%s: the row envelope has %lld blocks (0 .. %d): list the keyframes by ascending mnId", WHO, (long long)env,
                    ORBFE_EG_MAX_ENVELOPE_BLOCKS);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;

  // the workspace is an allocation of its own; its guard is declared before the call, so it is freed after the call has drained
  struct Workspace {
    void* p = nullptr;
    ~Workspace() {
      if (p) (void)hipFree(p);
    }
  } ws;
  HostCall c(WHO);
  const size_t o_prob = c.in(sizeof(orbfe_eg_problem)), o_v = c.in((size_t)n_kf * sizeof(orbfe_eg_vertex)),
               o_e = c.in((size_t)n_edges * sizeof(orbfe_eg_edge));
  const size_t o_res = c.out(sizeof(orbfe_eg_result)), o_s = c.out((size_t)n_kf * sizeof(orbfe_eg_sim3)), o_p = c.out((size_t)n_kf * 48);
  const size_t ws_bytes = eg_ws_bytes(n_kf, n_edges, (int)env);
  if ((rc = c.open())) return rc;
  if (ws_bytes && (rc = hip_status("essential graph: workspace", hipMalloc(&ws.p, ws_bytes)))) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  const orbfe_eg_problem prob = {0, n_kf, 0, n_edges};
  memcpy(h + o_prob, &prob, sizeof(prob));
  if (n_kf) memcpy(h + o_v, vertices, (size_t)n_kf * sizeof(orbfe_eg_vertex));
  if (n_edges) memcpy(h + o_e, edges, (size_t)n_edges * sizeof(orbfe_eg_edge));
  if ((rc = c.upload())) return rc;
  EgLaunch L;
  memset(&L, 0, sizeof(L));
  L.problems = (const orbfe_eg_problem*)(d + o_prob); L.vertices = (const orbfe_eg_vertex*)(d + o_v);
  L.edges = (const orbfe_eg_edge*)(d + o_e); L.kf_cap = n_kf; L.edge_cap = n_edges; L.env_cap = (int)env; L.flags = flags;
  L.sim3_out = (orbfe_eg_sim3*)(d + o_s); L.poses_out = (float*)(d + o_p); L.result = (orbfe_eg_result*)(d + o_res);
  L.workspace = (uint8_t*)ws.p;
  orbfe_launch_essential_graph(L, 1, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(result, h + o_res, sizeof(orbfe_eg_result));
  if (n_kf) memcpy(sim3_out, h + o_s, (size_t)n_kf * sizeof(orbfe_eg_sim3));
  if (n_kf) memcpy(poses_out, h + o_p, (size_t)n_kf * 48);
  if (result->status == ORBFE_EG_REFUSED) {   // the kernel's limits are the host's: unreachable unless the two drift apart
    orbfe_set_error("%s: refused on the device", WHO);
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
}

static bool correct_args_ok(const char* who, const void* points, int n_points, const void* ref, const void* from, const void* to, int n_tables,
                            const void* out) {
  if (n_points < 0 || n_points > EG_MAX_POINTS || n_tables < 0 || n_tables > ORBFE_EG_MAX_KEYFRAMES) {
    orbfe_set_error("%s: n_points %d (0 .. %d), n_tables %d (0 .. %d)", who, n_points, EG_MAX_POINTS, n_tables, ORBFE_EG_MAX_KEYFRAMES);
    return false;
  }
  if ((n_points > 0 && (!points || !ref || !out)) || (n_tables > 0 && (!from || !to))) {
    orbfe_set_error("%s: the arrays of a count > 0 are required", who);
    return false;
  }
  return true;
}

extern "C" int orbfe_sim3_correct_points_device(const float* d_points, int n_points, const int32_t* d_ref, const void* d_from, int from_stride,
                                                const orbfe_eg_sim3* d_to, int n_tables, float* d_points_out, void* stream) {
  const char* who = "sim3 correct points device";
  if (!correct_args_ok(who, d_points, n_points, d_ref, d_from, d_to, n_tables, d_points_out)) return ORBFE_ERR_INVALID;
  if (from_stride < (int)sizeof(orbfe_eg_sim3) || (from_stride & 7) || ((uintptr_t)d_from & 7) || ((uintptr_t)d_to & 7) ||
      ((uintptr_t)d_points & 3) || ((uintptr_t)d_ref & 3) || ((uintptr_t)d_points_out & 3)) {
    orbfe_set_error("%s: from_stride %d (>= 64, a multiple of 8); the tables 8-byte, the other arrays 4-byte aligned", who, from_stride);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  orbfe_launch_correct_points(d_points, n_points, d_ref, (const uint8_t*)d_from, from_stride, d_to, n_tables, d_points_out,
                              (hipStream_t)stream);
  return hip_status("sim3 correct points device: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_sim3_correct_points(const float* points, int n_points, const int32_t* ref, const orbfe_eg_sim3* from,
                                         const orbfe_eg_sim3* to, int n_tables, float* points_out) {
  const char* who = "sim3 correct points";
  if (!correct_args_ok(who, points, n_points, ref, from, to, n_tables, points_out)) return ORBFE_ERR_INVALID;
  for (int p = 0; p < n_points; p++)
    if (ref[p] >= n_tables) {
      orbfe_set_error("%s: ref[%d] = %d (< %d)", who, p, ref[p], n_tables);
      return ORBFE_ERR_INVALID;
    }
  for (int k = 0; k < n_tables; k++)
    if (!eg_record_ok(from[k]) || !eg_record_ok(to[k])) {
      orbfe_set_error("%s: table row %d: a record must be finite with s > 0 and a quaternion of non-zero norm", who, k);
      return ORBFE_ERR_INVALID;
    }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (n_points == 0) return ORBFE_OK;
  HostCall c(who);
  const size_t o_x = c.in((size_t)n_points * 12), o_r = c.in((size_t)n_points * 4), o_f = c.in((size_t)n_tables * sizeof(orbfe_eg_sim3)),
               o_t = c.in((size_t)n_tables * sizeof(orbfe_eg_sim3));
  const size_t o_out = c.out((size_t)n_points * 12);
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  memcpy(h + o_x, points, (size_t)n_points * 12);
  memcpy(h + o_r, ref, (size_t)n_points * 4);
  if (n_tables) memcpy(h + o_f, from, (size_t)n_tables * sizeof(orbfe_eg_sim3));
  if (n_tables) memcpy(h + o_t, to, (size_t)n_tables * sizeof(orbfe_eg_sim3));
  if ((rc = c.upload())) return rc;
  orbfe_launch_correct_points((const float*)(d + o_x), n_points, (const int32_t*)(d + o_r), d + o_f, (int)sizeof(orbfe_eg_sim3),
                              (const orbfe_eg_sim3*)(d + o_t), n_tables, (float*)(d + o_out), c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(points_out, h + o_out, (size_t)n_points * 12);
  return ORBFE_OK;
}
