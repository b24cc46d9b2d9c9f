// mapping.cpp -- C ABI of LocalMapping::CreateNewMapPoints (include/orbfe.h: orbfe_triangulate_matches*, orbfe_create_new_map_points).
// The entry points validate, stage and launch mapping_kernels.hip (and, for the chain, the search of bow_kernels.hip through the
// helpers orbfe_search_for_triangulation itself uses).  No CPU fallback: without a device all three are an error.
#include <string.h>

#include <algorithm>
#include <vector>

#include "host_internal.h"
#include "mapping_internal.h"
#include "match_internal.h"

#define TRI_MAX_ROWS 65535   // the descriptor limit of SearchForTriangulation (triangulation_match, bow_kernels.hip, packs a position into 16 bits)

static bool view_ok(const orbfe_tri_view* v, const char* what) {
  if (v->n_levels < 1 || v->n_levels > ORBFE_MAX_LEVELS) {
    orbfe_set_error("triangulation: n_levels %d of %s (1 .. %d)", v->n_levels, what, ORBFE_MAX_LEVELS);
    return false;
  }
  return true;
}

extern "C" int orbfe_triangulate_matches_batch_device(int K, const orbfe_tri_view* d_view1, const orbfe_keypoint* d_keys1,
                                                      const float* d_u_right1, const float* d_depth1, const int32_t* d_nA, int capA,
                                                      const orbfe_tri_view* d_view2, const orbfe_keypoint* d_keys2,
                                                      const float* d_u_right2, const float* d_depth2, const int32_t* d_nB, int capB,
                                                      const int32_t* d_matchA, orbfe_new_point* d_out, int32_t* d_n_new, void* stream) {
  if (!d_view1 || !d_keys1 || !d_nA || !d_view2 || !d_keys2 || !d_nB || !d_matchA || !d_out || !d_n_new) {
    orbfe_set_error("triangulation batch: views, keypoints, counts, matches, records and n_new are required (only u_right / depth may "
                    "be NULL)");
    return ORBFE_ERR_INVALID;
  }
  if (K < 0 || K > TRI_MAX_ROWS || capA < 1 || capA > TRI_MAX_ROWS || capB < 1 || capB > TRI_MAX_ROWS) {
    orbfe_set_error("triangulation batch: K %d (0 .. %d), capA %d, capB %d (1 .. %d)", K, TRI_MAX_ROWS, capA, capB, TRI_MAX_ROWS);
    return ORBFE_ERR_INVALID;
  }
  if ((d_u_right1 && !d_depth1) || (d_u_right2 && !d_depth2)) {
    orbfe_set_error("triangulation batch: u_right needs depth");
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_view1 & 3) || ((uintptr_t)d_keys1 & 3) || ((uintptr_t)d_u_right1 & 3) || ((uintptr_t)d_depth1 & 3) ||
      ((uintptr_t)d_nA & 3) || ((uintptr_t)d_view2 & 3) || ((uintptr_t)d_keys2 & 3) || ((uintptr_t)d_u_right2 & 3) ||
      ((uintptr_t)d_depth2 & 3) || ((uintptr_t)d_nB & 3) || ((uintptr_t)d_matchA & 3) || ((uintptr_t)d_out & 3) || ((uintptr_t)d_n_new & 3)) {
    orbfe_set_error("triangulation batch: records must be 4-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (K == 0) return ORBFE_OK;
  TriLaunch t;
  memset(&t, 0, sizeof(t));
  t.view1 = d_view1; t.keys1 = d_keys1; t.u_right1 = d_u_right1; t.depth1 = d_depth1; t.nA = d_nA; t.capA = capA;
  t.view2 = d_view2; t.keys2 = d_keys2; t.u_right2 = d_u_right2; t.depth2 = d_depth2; t.nB = d_nB; t.capB = capB;
  t.matchA = d_matchA; t.out = d_out;
  orbfe_launch_triangulate(t, K, (hipStream_t)stream);
  orbfe_launch_triangulate_count(d_out, d_nA, 0, capA, d_n_new, nullptr, 0, nullptr, K, (hipStream_t)stream);
  return hip_status("triangulation batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_triangulate_matches(const orbfe_tri_view* view1, const orbfe_keypoint* keys1, const float* u_right1,
                                         const float* depth1, int nA, const orbfe_tri_view* view2, const orbfe_keypoint* keys2,
                                         const float* u_right2, const float* depth2, int nB, const int32_t* matchA,
                                         orbfe_new_point* out, int* n_new) {
  if (!view1 || !view2 || !n_new) {
    orbfe_set_error("triangulation: both views and n_new are required");
    return ORBFE_ERR_INVALID;
  }
  if (nA < 0 || nA > TRI_MAX_ROWS || nB < 0 || nB > TRI_MAX_ROWS) {
    orbfe_set_error("triangulation: nA %d, nB %d (0 .. %d)", nA, nB, TRI_MAX_ROWS);
    return ORBFE_ERR_INVALID;
  }
  if (!view_ok(view1, "pKF1") || !view_ok(view2, "pKF2")) return ORBFE_ERR_INVALID;
  if ((u_right1 && !depth1) || (u_right2 && !depth2)) {
    orbfe_set_error("triangulation: u_right needs depth");
    return ORBFE_ERR_INVALID;
  }
  if ((nA > 0 && (!keys1 || !matchA || !out)) || (nB > 0 && !keys2)) {
    orbfe_set_error("triangulation: keys1, matchA and out are required for nA > 0, keys2 for nB > 0");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  *n_new = 0;
  if (nA == 0) return ORBFE_OK;
  const int capB = nB > 0 ? nB : 1;
  // [input, uploaded | output, downloaded]; u_right / depth have regions only when given, and reach the kernel as NULL otherwise
  const size_t b_u2 = u_right2 ? (size_t)capB * 4 : 0;
  HostCall c("triangulation");
  const size_t o_v1 = c.in(sizeof(orbfe_tri_view)), o_v2 = c.in(sizeof(orbfe_tri_view)), o_k1 = c.in((size_t)nA * sizeof(orbfe_keypoint)),
               o_u1 = c.in(u_right1 ? (size_t)nA * 4 : 0), o_d1 = c.in(u_right1 ? (size_t)nA * 4 : 0),
               o_k2 = c.in((size_t)capB * sizeof(orbfe_keypoint)), o_u2 = c.in(b_u2), o_d2 = c.in(b_u2), o_m = c.in((size_t)nA * 4);
  const size_t o_out = c.out((size_t)nA * sizeof(orbfe_new_point)), o_n = c.out(4);
  int rc;
  if ((rc = c.open())) return rc;
  memcpy(c.host(o_v1), view1, sizeof(orbfe_tri_view));
  memcpy(c.host(o_v2), view2, sizeof(orbfe_tri_view));
  memcpy(c.host(o_k1), keys1, (size_t)nA * sizeof(orbfe_keypoint));
  if (u_right1) {
    memcpy(c.host(o_u1), u_right1, (size_t)nA * 4);
    memcpy(c.host(o_d1), depth1, (size_t)nA * 4);
  }
  if (nB > 0) memcpy(c.host(o_k2), keys2, (size_t)nB * sizeof(orbfe_keypoint));
  if (nB > 0 && u_right2) {
    memcpy(c.host(o_u2), u_right2, (size_t)nB * 4);
    memcpy(c.host(o_d2), depth2, (size_t)nB * 4);
  }
  memcpy(c.host(o_m), matchA, (size_t)nA * 4);
  if ((rc = c.upload())) return rc;
  TriLaunch t;
  memset(&t, 0, sizeof(t));
  t.view1 = c.dev<const orbfe_tri_view>(o_v1); t.keys1 = c.dev<const orbfe_keypoint>(o_k1);
  t.u_right1 = u_right1 ? c.dev<const float>(o_u1) : nullptr; t.depth1 = u_right1 ? c.dev<const float>(o_d1) : nullptr;
  t.nA_host = nA; t.capA = nA;
  t.view2 = c.dev<const orbfe_tri_view>(o_v2); t.keys2 = c.dev<const orbfe_keypoint>(o_k2);
  t.u_right2 = u_right2 ? c.dev<const float>(o_u2) : nullptr; t.depth2 = u_right2 ? c.dev<const float>(o_d2) : nullptr;
  t.nB_host = nB; t.capB = capB;
  t.matchA = c.dev<const int32_t>(o_m); t.out = c.dev<orbfe_new_point>(o_out);
  orbfe_launch_triangulate(t, 1, c.stream);
  orbfe_launch_triangulate_count(t.out, nullptr, nA, nA, c.dev<int32_t>(o_n), nullptr, 0, nullptr, 1, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(out, c.host(o_out), (size_t)nA * sizeof(orbfe_new_point));
  *n_new = *c.host<const int32_t>(o_n);
  return ORBFE_OK;
}

extern "C" int orbfe_create_new_map_points(const orbfe_keypoint* keysA, const uint8_t* descA, const float* u_rightA, const float* depthA,
                                           uint8_t* has_mpA, int nA, const orbfe_featvec_node* nodesA, int n_nodesA,
                                           const int32_t* idxA, const orbfe_tri_view* viewA, const orbfe_tri_neighbor* neighbors, int K,
                                           int monocular, int only_stereo, int check_orientation, orbfe_new_point* points,
                                           int32_t* n_matches, int32_t* n_new) {
  if (!viewA || K < 0 || nA < 0 || nA > TRI_MAX_ROWS || n_nodesA < 0) {
    orbfe_set_error("create new map points: pKF1's view is required, K %d (>= 0), nA %d (0 .. %d), n_nodesA %d (>= 0)", K, nA, TRI_MAX_ROWS,
                    n_nodesA);
    return ORBFE_ERR_INVALID;
  }
  if (!view_ok(viewA, "pKF1")) return ORBFE_ERR_INVALID;
  if (K > 0 && (!neighbors || !n_matches || !n_new)) {
    orbfe_set_error("create new map points: neighbors, n_matches and n_new are required for K > 0");
    return ORBFE_ERR_INVALID;
  }
  if (nA > 0 && (!keysA || !descA || !has_mpA || (K > 0 && !points))) {
    orbfe_set_error("create new map points: keysA, descA, has_mpA and points are required for nA > 0");
    return ORBFE_ERR_INVALID;
  }
  if ((u_rightA && !depthA) || (n_nodesA > 0 && (!nodesA || !idxA))) {
    orbfe_set_error("create new map points: u_rightA needs depthA, n_nodesA > 0 needs nodesA and idxA");
    return ORBFE_ERR_INVALID;
  }
  for (int k = 0; k < K; k++) {
    const orbfe_tri_neighbor& N = neighbors[k];
    if (N.n < 0 || N.n > TRI_MAX_ROWS || N.n_nodes < 0 || (N.n > 0 && (!N.keys || !N.desc || !N.has_mp)) || (N.u_right && !N.depth) ||
        (N.n_nodes > 0 && (!N.nodes || !N.idx))) {
      orbfe_set_error("create new map points: neighbour %d: n %d (0 .. %d), n_nodes %d (>= 0); keys, desc, has_mp, nodes and idx are "
                      "required for their counts, u_right needs depth", k, N.n, TRI_MAX_ROWS, N.n_nodes);
      return ORBFE_ERR_INVALID;
    }
    if (!view_ok(&N.view, "a neighbour")) return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  for (int k = 0; k < K; k++) n_matches[k] = n_new[k] = 0;
  if (K == 0 || nA == 0) return ORBFE_OK;

  // per neighbour: the gate of :221-235, then the host half of the search
  std::vector<TriSearchPlan> plans((size_t)K);
  std::vector<uint8_t> gated((size_t)K, 0), active((size_t)K, 0);
  int totA = 0;
  for (int i = 0; i < n_nodesA; i++) totA = std::max(totA, nodesA[i].start + nodesA[i].count);
  for (int k = 0; k < K; k++) {
    const orbfe_tri_neighbor& N = neighbors[k];
    gated[k] = tri_baseline_too_short(viewA->Ow, N.view.Ow, monocular, N.view.mb, N.median_depth);
    if (gated[k] || N.n == 0 || n_nodesA == 0 || N.n_nodes == 0) continue;
    const int rc = orbfe_tri_search_plan(nA, nodesA, n_nodesA, idxA, N.n, N.nodes, N.n_nodes, N.idx, plans[k]);
    if (rc) {
      orbfe_set_error("create new map points: neighbour %d: malformed FeatureVector", k);
      return rc;
    }
    active[k] = !plans[k].pairs.empty();
  }

  size_t push_n = (size_t)nA;   // one scratch for all neighbours, which run one after the other: the largest plan's visits
  for (int k = 0; k < K; k++) push_n = std::max(push_n, (size_t)plans[k].push_cap);
  HostCall c("create new map points");
  const size_t o_vw1 = c.in(sizeof(orbfe_tri_view)), o_kA = c.in((size_t)nA * sizeof(orbfe_keypoint)), o_dA = c.in((size_t)nA * 32),
               o_uA = c.in((size_t)nA * 4), o_zA = c.in((size_t)nA * 4), o_iA = c.in((size_t)totA * 4), o_vA = c.in((size_t)nA),
               o_sA = c.in((size_t)nA), o_vw2 = c.in((size_t)K * sizeof(orbfe_tri_view)), o_mA = c.in((size_t)K * nA * 4),
               o_cnt = c.in((size_t)K * 256);
  struct NbOff { size_t pairs, keys, desc, ur, z, idx, valid, stereo; };
  std::vector<NbOff> nb((size_t)K);
  for (int k = 0; k < K; k++) {
    const orbfe_tri_neighbor& N = neighbors[k];
    const size_t n = (size_t)std::max(N.n, 1);
    nb[k].keys = c.in(n * sizeof(orbfe_keypoint));
    nb[k].ur = c.in(n * 4);
    nb[k].z = c.in(n * 4);
    if (!active[k]) continue;
    nb[k].pairs = c.in(plans[k].pairs.size() * sizeof(BowPair));
    nb[k].desc = c.in(n * 32);
    nb[k].idx = c.in((size_t)plans[k].totB * 4);
    nb[k].valid = c.in(n);
    nb[k].stereo = c.in(n);
  }
  const size_t o_pi = c.scratch(push_n * 4), o_pb = c.scratch(push_n);
  const size_t o_out = c.out((size_t)K * nA * sizeof(orbfe_new_point)), o_nn = c.out((size_t)K * 4), o_nm = c.out((size_t)K * 4);
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  const hipStream_t s = c.stream;
  // pKF1, once
  memcpy(h + o_vw1, viewA, sizeof(orbfe_tri_view));
  memcpy(h + o_kA, keysA, (size_t)nA * sizeof(orbfe_keypoint));
  memcpy(h + o_dA, descA, (size_t)nA * 32);
  if (u_rightA) {
    memcpy(h + o_uA, u_rightA, (size_t)nA * 4);
    memcpy(h + o_zA, depthA, (size_t)nA * 4);
  }
  if (totA > 0) memcpy(h + o_iA, idxA, (size_t)totA * 4);
  for (int i = 0; i < nA; i++) {   // candidate mask and stereo flag (ORBmatcher.cc:655-664)
    const uint8_t st = u_rightA && u_rightA[i] >= 0;
    h[o_sA + i] = st;
    h[o_vA + i] = !has_mpA[i] && (!only_stereo || st);
  }
  memset(h + o_mA, 0xff, (size_t)K * nA * 4);   // matchA of every neighbour: -1
  memset(h + o_cnt, 0, (size_t)K * 256);
  for (int k = 0; k < K; k++) {
    const orbfe_tri_neighbor& N = neighbors[k];
    memcpy(h + o_vw2 + (size_t)k * sizeof(orbfe_tri_view), &N.view, sizeof(orbfe_tri_view));
    if (N.n > 0) memcpy(h + nb[k].keys, N.keys, (size_t)N.n * sizeof(orbfe_keypoint));
    if (N.n > 0 && N.u_right) {
      memcpy(h + nb[k].ur, N.u_right, (size_t)N.n * 4);
      memcpy(h + nb[k].z, N.depth, (size_t)N.n * 4);
    }
    if (!active[k]) continue;
    memcpy(h + nb[k].pairs, plans[k].pairs.data(), plans[k].pairs.size() * sizeof(BowPair));
    memcpy(h + nb[k].desc, N.desc, (size_t)N.n * 32);
    memcpy(h + nb[k].idx, N.idx, (size_t)plans[k].totB * 4);
    for (int j = 0; j < N.n; j++) {   // :677-686
      const uint8_t st = N.u_right && N.u_right[j] >= 0;
      h[nb[k].stereo + j] = st;
      h[nb[k].valid + j] = !N.has_mp[j] && (!only_stereo || st);
    }
  }
  if ((rc = c.upload())) return rc;
  for (int k = 0; k < K; k++) {
    const orbfe_tri_neighbor& N = neighbors[k];
    int32_t* d_match = (int32_t*)(d + o_mA) + (size_t)k * nA;
    if (active[k]) {
      TriSearchBuffers b;
      b.pairs = (const BowPair*)(d + nb[k].pairs); b.n_pairs = (int)plans[k].pairs.size();
      b.descA = d + o_dA; b.descB = d + nb[k].desc;
      b.keysA = (const orbfe_keypoint*)(d + o_kA); b.keysB = (const orbfe_keypoint*)(d + nb[k].keys);
      b.idxA = (const int32_t*)(d + o_iA); b.idxB = (const int32_t*)(d + nb[k].idx);
      b.validA = d + o_vA; b.validB = d + nb[k].valid; b.stereoA = d + o_sA; b.stereoB = d + nb[k].stereo;
      b.matchA = d_match; b.counters = (int32_t*)(d + o_cnt + (size_t)k * 256);
      b.push_idx = (int32_t*)(d + o_pi); b.push_bin = d + o_pb;
      if ((rc = orbfe_tri_search_enqueue(b, &N.ep, check_orientation, plans[k].sequential, s))) return rc;
    }
    // a neighbour without a search still gets its rows written (all "no match"): its matchA is the uploaded -1
    TriLaunch t;
    memset(&t, 0, sizeof(t));
    t.view1 = (const orbfe_tri_view*)(d + o_vw1); t.keys1 = (const orbfe_keypoint*)(d + o_kA);
    t.u_right1 = u_rightA ? (const float*)(d + o_uA) : nullptr; t.depth1 = u_rightA ? (const float*)(d + o_zA) : nullptr;
    t.nA_host = nA; t.capA = nA;
    t.view2 = (const orbfe_tri_view*)(d + o_vw2) + k; t.keys2 = (const orbfe_keypoint*)(d + nb[k].keys);
    t.u_right2 = N.u_right ? (const float*)(d + nb[k].ur) : nullptr; t.depth2 = N.u_right ? (const float*)(d + nb[k].z) : nullptr;
    t.nB_host = N.n; t.capB = std::max(N.n, 1);
    t.matchA = d_match; t.out = (orbfe_new_point*)(d + o_out) + (size_t)k * nA;
    t.validA = d + o_vA;
    orbfe_launch_triangulate(t, 1, s);
  }
  orbfe_launch_triangulate_count((const orbfe_new_point*)(d + o_out), nullptr, nA, nA, (int32_t*)(d + o_nn), (const int32_t*)(d + o_cnt), 64,
                                 (int32_t*)(d + o_nm), K, s);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(points, h + o_out, (size_t)K * nA * sizeof(orbfe_new_point));
  memcpy(n_new, h + o_nn, (size_t)K * 4);
  memcpy(n_matches, h + o_nm, (size_t)K * 4);
  for (int k = 0; k < K; k++) {
    if (gated[k]) n_matches[k] = -1;
    for (int i = 0; i < nA; i++)
      if (points[(size_t)k * nA + i].code == ORBFE_TRI_OK) has_mpA[i] = 1;
  }
  return ORBFE_OK;
}
