// sim3.cpp -- C ABI of Sim3Solver (include/orbfe.h: orbfe_sim3_ransac_iterations, orbfe_sim3_solve, orbfe_sim3_solve_batch_device).
// The entry points validate, stage and launch sim3_kernels.hip.  No CPU fallback: without a device both solve forms are an error.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "host_internal.h"
#include "sim3_internal.h"

#define SIM3_MAX_PROBLEMS 65535   // grid.y

// Sim3Solver::SetRansacParameters (L/src/Sim3Solver.cc:112-136)
extern "C" int orbfe_sim3_ransac_iterations(int N, double probability, int min_inliers, int max_iterations) {
  if (N < 1 || min_inliers < 0 || min_inliers > N || max_iterations < 0 || !(probability > 0.0 && probability < 1.0)) {
    orbfe_set_error("sim3 ransac iterations: N %d (>= 1), min_inliers %d (0 .. N), max_iterations %d (>= 0), probability %g (inside 0 .. 1)",
                    N, min_inliers, max_iterations, probability);
    return ORBFE_ERR_INVALID;
  }
  const float epsilon = (float)min_inliers / N;
  return ransac_iterations(min_inliers == N, probability, epsilon, max_iterations);
}

extern "C" int orbfe_sim3_solve_batch_device(int P, const orbfe_sim3_view* d_view1, const orbfe_sim3_view* d_view2,
                                             const orbfe_sim3_pair* d_pairs, const int32_t* d_n, int cap, const int32_t* d_triples,
                                             const int32_t* d_H, int h_cap, const int32_t* d_fix_scale, const int32_t* d_min_inliers,
                                             orbfe_sim3_hypothesis* d_hyps, uint64_t* d_words, orbfe_sim3_result* d_result,
                                             uint64_t* d_result_mask, void* stream) {
  if (!d_view1 || !d_view2 || !d_pairs || !d_n || !d_triples || !d_H || !d_fix_scale || !d_min_inliers || !d_hyps || !d_words || !d_result ||
      !d_result_mask) {
    orbfe_set_error("sim3 batch: every pointer is required");
    return ORBFE_ERR_INVALID;
  }
  if (P < 0 || P > SIM3_MAX_PROBLEMS || cap < 1 || cap > ORBFE_SIM3_MAX_PAIRS || h_cap < 1 || h_cap > ORBFE_SIM3_MAX_HYPOTHESES) {
    orbfe_set_error("sim3 batch: P %d (0 .. %d), cap %d (1 .. %d), h_cap %d (1 .. %d)", P, SIM3_MAX_PROBLEMS, cap, ORBFE_SIM3_MAX_PAIRS, h_cap,
                    ORBFE_SIM3_MAX_HYPOTHESES);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_view1 & 3) || ((uintptr_t)d_view2 & 3) || ((uintptr_t)d_pairs & 3) || ((uintptr_t)d_n & 3) || ((uintptr_t)d_triples & 3) ||
      ((uintptr_t)d_H & 3) || ((uintptr_t)d_fix_scale & 3) || ((uintptr_t)d_min_inliers & 3) || ((uintptr_t)d_hyps & 3) ||
      ((uintptr_t)d_result & 3) || ((uintptr_t)d_words & 7) || ((uintptr_t)d_result_mask & 7)) {
    orbfe_set_error("sim3 batch: records must be 4-byte aligned, inlier words 8-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (P == 0) return ORBFE_OK;
  Sim3Launch L;
  memset(&L, 0, sizeof(L));
  L.view1 = d_view1; L.view2 = d_view2; L.pairs = d_pairs; L.n = d_n; L.cap = cap;
  L.triples = d_triples; L.H = d_H; L.h_cap = h_cap; L.fix_scale = d_fix_scale; L.min_inliers = d_min_inliers;
  L.hyps = d_hyps; L.words = d_words; L.result = d_result; L.mask = d_result_mask;
  orbfe_launch_sim3_hypotheses(L, P, (hipStream_t)stream);
  orbfe_launch_sim3_select(L, P, (hipStream_t)stream);
  return hip_status("sim3 batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_sim3_solve(const orbfe_sim3_view* view1, const orbfe_sim3_view* view2, const orbfe_sim3_pair* pairs, int n,
                                const int32_t* triples, int H, int fix_scale, int min_inliers, orbfe_sim3_hypothesis* hyps,
                                uint64_t* words, orbfe_sim3_result* result, uint64_t* result_mask) {
  if (!view1 || !view2 || !result || !result_mask) {
    orbfe_set_error("sim3 solve: both views, result and result_mask are required");
    return ORBFE_ERR_INVALID;
  }
  if (n < 0 || n > ORBFE_SIM3_MAX_PAIRS || H < 0 || H > ORBFE_SIM3_MAX_HYPOTHESES || min_inliers < 0) {
    orbfe_set_error("sim3 solve: n %d (0 .. %d), H %d (0 .. %d), min_inliers %d (>= 0)", n, ORBFE_SIM3_MAX_PAIRS, H, ORBFE_SIM3_MAX_HYPOTHESES,
                    min_inliers);
    return ORBFE_ERR_INVALID;
  }
  if ((n > 0 && !pairs) || (H > 0 && !triples)) {
    orbfe_set_error("sim3 solve: pairs are required for n > 0, triples for H > 0");
    return ORBFE_ERR_INVALID;
  }
  for (int h = 0; h < H; h++)
    if (!sim3_triple_ok(triples[3 * h], triples[3 * h + 1], triples[3 * h + 2], n)) {
      orbfe_set_error("sim3 solve: triple %d (%d, %d, %d): indices must lie in [0, %d) and differ", h, triples[3 * h], triples[3 * h + 1],
                      triples[3 * h + 2], n);
      return ORBFE_ERR_INVALID;
    }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  const size_t n_words = ((size_t)n + 63) / 64;
  if (n < 3 || n < min_inliers || H == 0) {   // :144-147: nothing is evaluated, nothing is launched
    memset(result, 0, sizeof(*result));
    result->returned = result->best = -1;
    memset(result_mask, 0, n_words * 8);
    if (hyps && H > 0) memset(hyps, 0, (size_t)H * sizeof(*hyps));
    if (words && H > 0) memset(words, 0, (size_t)H * n_words * 8);
    return ORBFE_OK;
  }
  // the optional outputs sit behind the result so that a caller who skips them also skips their bytes in the download
  HostCall c("sim3 solve");
  const size_t o_v1 = c.in(sizeof(orbfe_sim3_view)), o_v2 = c.in(sizeof(orbfe_sim3_view)), o_scal = c.in(16),
               o_pairs = c.in((size_t)n * sizeof(orbfe_sim3_pair)), o_tri = c.in((size_t)H * 12);
  const size_t o_res = c.out(sizeof(orbfe_sim3_result)), o_mask = c.out(n_words * 8), o_words = c.out((size_t)H * n_words * 8),
               o_hyps = c.out((size_t)H * sizeof(orbfe_sim3_hypothesis));
  const size_t out_end = hyps ? c.total() : (words ? o_hyps : o_words);
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  memcpy(h + o_v1, view1, sizeof(orbfe_sim3_view));
  memcpy(h + o_v2, view2, sizeof(orbfe_sim3_view));
  const int32_t scal[4] = {n, H, fix_scale != 0, min_inliers};
  memcpy(h + o_scal, scal, sizeof(scal));
  memcpy(h + o_pairs, pairs, (size_t)n * sizeof(orbfe_sim3_pair));
  memcpy(h + o_tri, triples, (size_t)H * 12);
  if ((rc = c.upload())) return rc;
  Sim3Launch L;
  memset(&L, 0, sizeof(L));
  const int32_t* d_scal = (const int32_t*)(d + o_scal);
  L.view1 = (const orbfe_sim3_view*)(d + o_v1); L.view2 = (const orbfe_sim3_view*)(d + o_v2);
  L.pairs = (const orbfe_sim3_pair*)(d + o_pairs); L.n = d_scal; L.cap = n;
  L.triples = (const int32_t*)(d + o_tri); L.H = d_scal + 1; L.h_cap = H; L.fix_scale = d_scal + 2; L.min_inliers = d_scal + 3;
  L.hyps = (orbfe_sim3_hypothesis*)(d + o_hyps); L.words = (uint64_t*)(d + o_words);
  L.result = (orbfe_sim3_result*)(d + o_res); L.mask = (uint64_t*)(d + o_mask);
  orbfe_launch_sim3_hypotheses(L, 1, c.stream);
  orbfe_launch_sim3_select(L, 1, c.stream);
  if ((rc = c.finish(out_end - o_res))) return rc;
  memcpy(result, h + o_res, sizeof(*result));
  memcpy(result_mask, h + o_mask, n_words * 8);
  if (words) memcpy(words, h + o_words, (size_t)H * n_words * 8);
  if (hyps) memcpy(hyps, h + o_hyps, (size_t)H * sizeof(*hyps));
  return ORBFE_OK;
}
