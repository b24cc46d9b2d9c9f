// initializer.cpp -- C ABI of Initializer::Initialize (include/orbfe.h: orbfe_initializer_initialize,
// orbfe_initializer_workspace_bytes, orbfe_initializer_initialize_batch_device).  The entry points validate, stage and launch
// initializer_kernels.hip.  No CPU fallback: without a device both forms are an error.
#include <string.h>

#include <algorithm>

#include "host_internal.h"
#include "initializer_internal.h"

#define INI_MAX_PROBLEMS 65535   // grid.y / grid.z

// the workspace of P problems of `cap` keypoints: headers, match coordinates, match indices
struct IniWorkspace {
  size_t header, mxy, mi1, total;
  IniWorkspace(int P, int cap) {
    Layout l;
    header = l.add((size_t)P * sizeof(IniHeader));
    mxy = l.add((size_t)P * cap * sizeof(float4));
    mi1 = l.add((size_t)P * cap * sizeof(int32_t));
    total = l.off;
  }
};

extern "C" int orbfe_initializer_workspace_bytes(int P, int cap, size_t* bytes) {
  if (!bytes || P < 0 || P > INI_MAX_PROBLEMS || cap < 1 || cap > ORBFE_INIT_MAX_MATCHES) {
    orbfe_set_error("initializer workspace: P %d (0 .. %d), cap %d (1 .. %d), bytes is required", P, INI_MAX_PROBLEMS, cap,
                    ORBFE_INIT_MAX_MATCHES);
    return ORBFE_ERR_INVALID;
  }
  *bytes = IniWorkspace(P, cap).total;
  return ORBFE_OK;
}

extern "C" int orbfe_initializer_initialize_batch_device(int P, const orbfe_init_params* d_params, const float* d_keys1,
                                                         const int32_t* d_n1, const float* d_keys2, const int32_t* d_n2, int cap,
                                                         const int32_t* d_matches12, const int32_t* d_sets, const int32_t* d_H, int h_cap,
                                                         orbfe_init_result* d_result, float* d_P3D, uint64_t* d_triangulated,
                                                         uint64_t* d_inlier_words, orbfe_init_hypothesis* d_hyps, uint64_t* d_words,
                                                         orbfe_init_candidate* d_candidates, void* d_workspace, size_t workspace_bytes,
                                                         void* stream) {
  if (!d_params || !d_keys1 || !d_n1 || !d_keys2 || !d_n2 || !d_matches12 || !d_sets || !d_H || !d_result || !d_P3D || !d_triangulated ||
      !d_inlier_words || !d_hyps || !d_words || !d_candidates || !d_workspace) {
    orbfe_set_error("initializer batch: every pointer is required");
    return ORBFE_ERR_INVALID;
  }
  if (P < 0 || P > INI_MAX_PROBLEMS || cap < 1 || cap > ORBFE_INIT_MAX_MATCHES || h_cap < 1 || h_cap > ORBFE_INIT_MAX_HYPOTHESES) {
    orbfe_set_error("initializer batch: P %d (0 .. %d), cap %d (1 .. %d), h_cap %d (1 .. %d)", P, INI_MAX_PROBLEMS, cap,
                    ORBFE_INIT_MAX_MATCHES, h_cap, ORBFE_INIT_MAX_HYPOTHESES);
    return ORBFE_ERR_INVALID;
  }
  const IniWorkspace ws(P, cap);
  if (workspace_bytes < ws.total) {
    orbfe_set_error("initializer batch: workspace of %zu bytes, %zu needed (orbfe_initializer_workspace_bytes)", workspace_bytes, ws.total);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_params & 3) || ((uintptr_t)d_keys1 & 3) || ((uintptr_t)d_n1 & 3) || ((uintptr_t)d_keys2 & 3) || ((uintptr_t)d_n2 & 3) ||
      ((uintptr_t)d_matches12 & 3) || ((uintptr_t)d_sets & 3) || ((uintptr_t)d_H & 3) || ((uintptr_t)d_result & 3) || ((uintptr_t)d_P3D & 3) ||
      ((uintptr_t)d_hyps & 3) || ((uintptr_t)d_candidates & 3) || ((uintptr_t)d_triangulated & 7) || ((uintptr_t)d_inlier_words & 7) ||
      ((uintptr_t)d_words & 7) || ((uintptr_t)d_workspace & 15)) {
    orbfe_set_error("initializer batch: records must be 4-byte aligned, words 8-byte, the workspace 16-byte");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (P == 0) return ORBFE_OK;
  IniLaunch L;
  memset(&L, 0, sizeof(L));
  L.params = d_params; L.keys1 = d_keys1; L.keys2 = d_keys2; L.n1 = d_n1; L.n2 = d_n2; L.cap = cap; L.matches12 = d_matches12;
  L.sets = d_sets; L.H = d_H; L.h_cap = h_cap; L.result = d_result; L.P3D = d_P3D; L.triangulated = d_triangulated;
  L.inlier_words = d_inlier_words; L.hyps = d_hyps; L.words = d_words; L.cands = d_candidates;
  uint8_t* w = (uint8_t*)d_workspace;
  L.header = (IniHeader*)(w + ws.header); L.mxy = (float4*)(w + ws.mxy); L.mi1 = (int32_t*)(w + ws.mi1);
  orbfe_launch_initializer(L, P, (hipStream_t)stream);
  return hip_status("initializer batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_initializer_initialize(const orbfe_init_params* params, const float* keys1, int n1, const float* keys2, int n2,
                                            const int32_t* matches12, const int32_t* sets, int H, orbfe_init_result* result, float* P3D,
                                            uint64_t* triangulated, uint64_t* inlier_words, orbfe_init_hypothesis* hyps_h,
                                            orbfe_init_hypothesis* hyps_f, uint64_t* words_h, uint64_t* words_f,
                                            orbfe_init_candidate* candidates) {
  if (!params || !result) {
    orbfe_set_error("initializer: params and result are required");
    return ORBFE_ERR_INVALID;
  }
  if (n1 < 0 || n1 > ORBFE_INIT_MAX_MATCHES || n2 < 0 || n2 > ORBFE_INIT_MAX_MATCHES || H < 0 || H > ORBFE_INIT_MAX_HYPOTHESES) {
    orbfe_set_error("initializer: n1 %d, n2 %d (0 .. %d), H %d (0 .. %d)", n1, n2, ORBFE_INIT_MAX_MATCHES, H, ORBFE_INIT_MAX_HYPOTHESES);
    return ORBFE_ERR_INVALID;
  }
  if ((n1 > 0 && (!keys1 || !matches12 || !P3D || !triangulated || !inlier_words)) || (n2 > 0 && !keys2) || (H > 0 && !sets)) {
    orbfe_set_error("initializer: keys1, matches12, P3D, triangulated and inlier_words are required for n1 > 0, keys2 for n2 > 0, sets for H > 0");
    return ORBFE_ERR_INVALID;
  }
  int N = 0;
  for (int i = 0; i < n1; i++) {
    if (matches12[i] >= n2) {
      orbfe_set_error("initializer: matches12[%d] = %d, the current frame has %d keypoints", i, matches12[i], n2);
      return ORBFE_ERR_INVALID;
    }
    N += matches12[i] >= 0;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  const int cap = std::max(1, std::max(n1, n2)), h_cap = std::max(1, H);
  const size_t W = ((size_t)cap + 63) / 64, n1_words = ((size_t)n1 + 63) / 64;
  if (N < 8) {   // no set of eight exists: nothing is launched
    memset(result, 0, sizeof(*result));
    result->best_h = result->best_f = result->best_candidate = -1;
    result->n_matches = N;
    result->reason = ORBFE_INIT_FEW_MATCHES;
    if (n1 > 0) {
      memset(P3D, 0, (size_t)n1 * 12);
      memset(triangulated, 0, n1_words * 8);
      memset(inlier_words, 0, n1_words * 8);
    }
    if (hyps_h && H > 0) memset(hyps_h, 0, (size_t)H * sizeof(*hyps_h));
    if (hyps_f && H > 0) memset(hyps_f, 0, (size_t)H * sizeof(*hyps_f));
    if (words_h && H > 0) memset(words_h, 0, (size_t)H * n1_words * 8);
    if (words_f && H > 0) memset(words_f, 0, (size_t)H * n1_words * 8);
    if (candidates) memset(candidates, 0, 8 * sizeof(*candidates));
    return ORBFE_OK;
  }
  // exactly the batch form with P = 1; the optional outputs sit behind the others so that a caller who skips them also skips their
  // bytes in the download
  const IniWorkspace ws(1, cap);
  HostCall c("initializer");
  const size_t o_par = c.in(sizeof(orbfe_init_params)), o_scal = c.in(16), o_k1 = c.in((size_t)cap * 8), o_k2 = c.in((size_t)cap * 8),
               o_m = c.in((size_t)cap * 4), o_sets = c.in((size_t)h_cap * 32);
  const size_t o_ws = c.scratch(ws.total);
  const size_t o_res = c.out(sizeof(orbfe_init_result)), o_p3d = c.out((size_t)cap * 12), o_tri = c.out(W * 8), o_inl = c.out(W * 8),
               o_cand = c.out(8 * sizeof(orbfe_init_candidate)), o_hyps = c.out((size_t)2 * h_cap * sizeof(orbfe_init_hypothesis)),
               o_words = c.out((size_t)2 * h_cap * W * 8);
  const bool want_words = words_h || words_f, want_hyps = hyps_h || hyps_f;
  const size_t out_end = want_words ? c.total() : (want_hyps ? o_words : (candidates ? o_hyps : o_cand));
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  memcpy(h + o_par, params, sizeof(*params));
  const int32_t scal[4] = {n1, n2, H, 0};
  memcpy(h + o_scal, scal, sizeof(scal));
  memset(h + o_k1, 0, (size_t)cap * 8);
  memset(h + o_k2, 0, (size_t)cap * 8);
  memset(h + o_m, 0xff, (size_t)cap * 4);
  memset(h + o_sets, 0, (size_t)h_cap * 32);
  if (n1 > 0) memcpy(h + o_k1, keys1, (size_t)n1 * 8);
  if (n2 > 0) memcpy(h + o_k2, keys2, (size_t)n2 * 8);
  if (n1 > 0) memcpy(h + o_m, matches12, (size_t)n1 * 4);
  if (H > 0) memcpy(h + o_sets, sets, (size_t)H * 32);
  if ((rc = c.upload())) return rc;
  IniLaunch L;
  memset(&L, 0, sizeof(L));
  const int32_t* d_scal = (const int32_t*)(d + o_scal);
  L.params = (const orbfe_init_params*)(d + o_par); L.keys1 = (const float*)(d + o_k1); L.keys2 = (const float*)(d + o_k2);
  L.n1 = d_scal; L.n2 = d_scal + 1; L.cap = cap; L.matches12 = (const int32_t*)(d + o_m);
  L.sets = (const int32_t*)(d + o_sets); L.H = d_scal + 2; L.h_cap = h_cap;
  L.result = (orbfe_init_result*)(d + o_res); L.P3D = (float*)(d + o_p3d); L.triangulated = (uint64_t*)(d + o_tri);
  L.inlier_words = (uint64_t*)(d + o_inl); L.hyps = (orbfe_init_hypothesis*)(d + o_hyps); L.words = (uint64_t*)(d + o_words);
  L.cands = (orbfe_init_candidate*)(d + o_cand);
  L.header = (IniHeader*)(d + o_ws + ws.header); L.mxy = (float4*)(d + o_ws + ws.mxy); L.mi1 = (int32_t*)(d + o_ws + ws.mi1);
  orbfe_launch_initializer(L, 1, c.stream);
  if ((rc = c.finish(out_end - o_res))) return rc;
  memcpy(result, h + o_res, sizeof(*result));
  memcpy(P3D, h + o_p3d, (size_t)n1 * 12);
  memcpy(triangulated, h + o_tri, n1_words * 8);
  memcpy(inlier_words, h + o_inl, n1_words * 8);
  if (candidates) memcpy(candidates, h + o_cand, 8 * sizeof(*candidates));
  const orbfe_init_hypothesis* hh = (const orbfe_init_hypothesis*)(h + o_hyps);
  if (hyps_h && H > 0) memcpy(hyps_h, hh, (size_t)H * sizeof(*hh));
  if (hyps_f && H > 0) memcpy(hyps_f, hh + h_cap, (size_t)H * sizeof(*hh));
  const uint64_t* hw = (const uint64_t*)(h + o_words);
  const size_t n_words = ((size_t)N + 63) / 64;
  for (int m = 0; m < 2; m++) {
    uint64_t* dst = m ? words_f : words_h;
    if (!dst) continue;
    for (int k = 0; k < H; k++) {   // the device rows are W apart and written up to ceil(N / 64); the caller's rows are ceil(n1 / 64)
      memset(dst + (size_t)k * n1_words, 0, n1_words * 8);
      memcpy(dst + (size_t)k * n1_words, hw + ((size_t)m * h_cap + k) * W, n_words * 8);
    }
  }
  return ORBFE_OK;
}
