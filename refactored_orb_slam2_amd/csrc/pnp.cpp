// pnp.cpp -- C ABI of PnPsolver (include/orbfe.h: orbfe_pnp_ransac_parameters, orbfe_pnp_solve, orbfe_pnp_solve_batch_device).
// The entry points validate, stage and launch pnp_kernels.hip.  No CPU fallback: without a device both solve forms are an error.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "host_internal.h"
#include "pnp_internal.h"

#define PNP_MAX_PROBLEMS 65535   // grid.y

// PnPsolver::SetRansacParameters (L/src/PnPsolver.cc:119-151)
extern "C" int orbfe_pnp_ransac_parameters(int N, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                                           int32_t* min_inliers_out, int32_t* iterations_out, float* epsilon_out) {
  if (N < 1 || min_inliers < 0 || max_iterations < 0 || min_set != 4 || !(probability > 0.0 && probability < 1.0) ||
      !(epsilon >= 0.0f && epsilon <= 1.0f) || !min_inliers_out || !iterations_out || !epsilon_out) {
    orbfe_set_error("pnp ransac parameters: N %d (>= 1), min_inliers %d (>= 0), max_iterations %d (>= 0), min_set %d (4), probability %g "
                    "(inside 0 .. 1), epsilon %g (0 .. 1), three outputs", N, min_inliers, max_iterations, min_set, probability, (double)epsilon);
    return ORBFE_ERR_INVALID;
  }
  int n_min = (int)((float)N * epsilon);   // int = int * float: the float product, truncated (:133)
  if (n_min < min_inliers) n_min = min_inliers;
  if (n_min < min_set) n_min = min_set;
  if (epsilon < (float)n_min / N) epsilon = (float)n_min / N;
  *min_inliers_out = n_min;
  *iterations_out = ransac_iterations(n_min == N, probability, epsilon, max_iterations);
  *epsilon_out = epsilon;
  return ORBFE_OK;
}

extern "C" int orbfe_pnp_solve_batch_device(int P, const orbfe_pnp_camera* d_camera, const orbfe_pnp_point* d_points, const int32_t* d_n,
                                            int cap, const int32_t* d_sets, const int32_t* d_H, int h_cap, const int32_t* d_min_inliers,
                                            orbfe_pnp_hypothesis* d_hyps, uint64_t* d_words, orbfe_pnp_refine* d_refines,
                                            uint64_t* d_refine_words, orbfe_pnp_diag* d_diag, orbfe_pnp_diag* d_refine_diag,
                                            orbfe_pnp_result* d_result, uint64_t* d_result_mask, void* stream) {
  if (!d_camera || !d_points || !d_n || !d_sets || !d_H || !d_min_inliers || !d_hyps || !d_words || !d_refines || !d_refine_words || !d_result ||
      !d_result_mask) {
    orbfe_set_error("pnp batch: every pointer but the two diagnostics is required");
    return ORBFE_ERR_INVALID;
  }
  if (P < 0 || P > PNP_MAX_PROBLEMS || cap < 1 || cap > ORBFE_PNP_MAX_POINTS || h_cap < 1 || h_cap > ORBFE_PNP_MAX_HYPOTHESES) {
    orbfe_set_error("pnp batch: P %d (0 .. %d), cap %d (1 .. %d), h_cap %d (1 .. %d)", P, PNP_MAX_PROBLEMS, cap, ORBFE_PNP_MAX_POINTS, h_cap,
                    ORBFE_PNP_MAX_HYPOTHESES);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_camera & 3) || ((uintptr_t)d_points & 3) || ((uintptr_t)d_n & 3) || ((uintptr_t)d_sets & 3) || ((uintptr_t)d_H & 3) ||
      ((uintptr_t)d_min_inliers & 3) || ((uintptr_t)d_result & 3) || ((uintptr_t)d_hyps & 7) || ((uintptr_t)d_words & 7) ||
      ((uintptr_t)d_refines & 7) || ((uintptr_t)d_refine_words & 7) || ((uintptr_t)d_diag & 7) || ((uintptr_t)d_refine_diag & 7) ||
      ((uintptr_t)d_result_mask & 7)) {
    orbfe_set_error("pnp batch: records with doubles and inlier words must be 8-byte aligned, the others 4-byte");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (P == 0) return ORBFE_OK;
  PnpLaunch L;
  memset(&L, 0, sizeof(L));
  L.camera = d_camera; L.points = d_points; L.n = d_n; L.cap = cap; L.sets = d_sets; L.H = d_H; L.h_cap = h_cap; L.min_inliers = d_min_inliers;
  L.hyps = d_hyps; L.words = d_words; L.refines = d_refines; L.refine_words = d_refine_words; L.diag = d_diag; L.refine_diag = d_refine_diag;
  L.result = d_result; L.mask = d_result_mask;
  orbfe_launch_pnp_hypotheses(L, P, (hipStream_t)stream);
  orbfe_launch_pnp_refine(L, P, (hipStream_t)stream);
  orbfe_launch_pnp_select(L, P, (hipStream_t)stream);
  return hip_status("pnp batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_pnp_solve(const orbfe_pnp_camera* camera, const orbfe_pnp_point* points, int n, const int32_t* sets, int min_set, int H,
                               int min_inliers, orbfe_pnp_hypothesis* hyps, uint64_t* words, orbfe_pnp_refine* refines,
                               uint64_t* refine_words, orbfe_pnp_diag* diag, orbfe_pnp_diag* refine_diag, orbfe_pnp_result* result,
                               uint64_t* result_mask) {
  if (!camera || !result || !result_mask) {
    orbfe_set_error("pnp solve: camera, result and result_mask are required");
    return ORBFE_ERR_INVALID;
  }
  if (n < 0 || n > ORBFE_PNP_MAX_POINTS || H < 0 || H > ORBFE_PNP_MAX_HYPOTHESES || min_inliers < 4 || min_set != 4) {
    orbfe_set_error("pnp solve: n %d (0 .. %d), H %d (0 .. %d), min_inliers %d (>= 4), min_set %d (4)", n, ORBFE_PNP_MAX_POINTS, H,
                    ORBFE_PNP_MAX_HYPOTHESES, min_inliers, min_set);
    return ORBFE_ERR_INVALID;
  }
  if ((n > 0 && !points) || (H > 0 && !sets)) {
    orbfe_set_error("pnp solve: points are required for n > 0, sets for H > 0");
    return ORBFE_ERR_INVALID;
  }
  for (int h = 0; h < H; h++)
    if (!pnp_set_ok(sets[4 * h], sets[4 * h + 1], sets[4 * h + 2], sets[4 * h + 3], n)) {
      orbfe_set_error("pnp solve: set %d (%d, %d, %d, %d): indices must lie in [0, %d) and differ", h, sets[4 * h], sets[4 * h + 1],
                      sets[4 * h + 2], sets[4 * h + 3], n);
      return ORBFE_ERR_INVALID;
    }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  const size_t n_words = ((size_t)n + 63) / 64, hs = (size_t)H;
  if (n < min_inliers || H == 0) {   // :171-174: nothing is evaluated, nothing is launched
    memset(result, 0, sizeof(*result));
    result->returned = result->best = -1;
    memset(result_mask, 0, n_words * 8);
    if (hyps && H > 0) memset(hyps, 0, hs * sizeof(*hyps));
    if (words && H > 0) memset(words, 0, hs * n_words * 8);
    if (refines && H > 0) memset(refines, 0, hs * sizeof(*refines));
    if (refine_words && H > 0) memset(refine_words, 0, hs * n_words * 8);
    if (diag && H > 0) memset(diag, 0, hs * sizeof(*diag));
    if (refine_diag && H > 0) memset(refine_diag, 0, hs * sizeof(*refine_diag));
    return ORBFE_OK;
  }
  // The records the selection reads stay on the device whether or not the caller wants them; the optional outputs lie behind the
  // result in the order of their likely use, and the download ends behind the last one that is wanted.
  HostCall c("pnp solve");
  const size_t o_cam = c.in(sizeof(orbfe_pnp_camera)), o_scal = c.in(16), o_pts = c.in((size_t)n * sizeof(orbfe_pnp_point)),
               o_sets = c.in(hs * 16);
  const size_t o_res = c.out(sizeof(orbfe_pnp_result)), o_mask = c.out(n_words * 8), o_hyps = c.out(hs * sizeof(orbfe_pnp_hypothesis)),
               o_words = c.out(hs * n_words * 8), o_ref = c.out(hs * sizeof(orbfe_pnp_refine)), o_rwords = c.out(hs * n_words * 8),
               o_diag = c.out(hs * sizeof(orbfe_pnp_diag)), o_rdiag = c.out(hs * sizeof(orbfe_pnp_diag));
  const size_t out_end = refine_diag ? c.total() : diag ? o_rdiag : refine_words ? o_diag : refines ? o_rwords : words ? o_ref : hyps ? o_words
                                                                                                                                       : o_hyps;
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  memcpy(h + o_cam, camera, sizeof(orbfe_pnp_camera));
  const int32_t scal[4] = {n, H, min_inliers, 0};
  memcpy(h + o_scal, scal, sizeof(scal));
  memcpy(h + o_pts, points, (size_t)n * sizeof(orbfe_pnp_point));
  memcpy(h + o_sets, sets, hs * 16);
  if ((rc = c.upload())) return rc;
  // rows of hypotheses without a refine come back zero
  if ((rc = c.status(hipMemsetAsync(d + o_ref, 0, o_diag - o_ref, c.stream)))) return rc;
  if (refine_diag && (rc = c.status(hipMemsetAsync(d + o_rdiag, 0, c.total() - o_rdiag, c.stream)))) return rc;
  PnpLaunch L;
  memset(&L, 0, sizeof(L));
  const int32_t* d_scal = (const int32_t*)(d + o_scal);
  L.camera = (const orbfe_pnp_camera*)(d + o_cam); L.points = (const orbfe_pnp_point*)(d + o_pts); L.n = d_scal; L.cap = n;
  L.sets = (const int32_t*)(d + o_sets); L.H = d_scal + 1; L.h_cap = H; L.min_inliers = d_scal + 2;
  L.hyps = (orbfe_pnp_hypothesis*)(d + o_hyps); L.words = (uint64_t*)(d + o_words);
  L.refines = (orbfe_pnp_refine*)(d + o_ref); L.refine_words = (uint64_t*)(d + o_rwords);
  L.diag = diag ? (orbfe_pnp_diag*)(d + o_diag) : nullptr; L.refine_diag = refine_diag ? (orbfe_pnp_diag*)(d + o_rdiag) : nullptr;
  L.result = (orbfe_pnp_result*)(d + o_res); L.mask = (uint64_t*)(d + o_mask);
  orbfe_launch_pnp_hypotheses(L, 1, c.stream);
  orbfe_launch_pnp_refine(L, 1, c.stream);
  orbfe_launch_pnp_select(L, 1, c.stream);
  if ((rc = c.finish(out_end - o_res))) return rc;
  memcpy(result, h + o_res, sizeof(*result));
  memcpy(result_mask, h + o_mask, n_words * 8);
  if (hyps) memcpy(hyps, h + o_hyps, hs * sizeof(*hyps));
  if (words) memcpy(words, h + o_words, hs * n_words * 8);
  if (refines) memcpy(refines, h + o_ref, hs * sizeof(*refines));
  if (refine_words) memcpy(refine_words, h + o_rwords, hs * n_words * 8);
  if (diag) memcpy(diag, h + o_diag, hs * sizeof(*diag));
  if (refine_diag) memcpy(refine_diag, h + o_rdiag, hs * sizeof(*refine_diag));
  return ORBFE_OK;
}
