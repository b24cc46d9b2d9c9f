// host_arith.cpp -- csrc/pnp_internal.h compiled for the HOST: the loops that pnp_kernels.hip spreads over workgroups, waves and
// lanes (here one lane does every item, in item order), so that the arithmetic the kernels execute can be compared with the numpy
// yardstick on a machine without a GPU (tests/test_pnp_cpu.py).  Same flags as the library (-ffp-contract=off).
#include <string.h>

#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/pnp_internal.h"

static int check_inliers(const PnpWork& w, int winner, const PnpCamera& K, const orbfe_pnp_point* pts, int n, uint64_t* row) {
  int count = 0;
  for (int i = 0; i < n; i++)
    if (pnp_is_inlier(w.st[winner].R, w.st[winner].t, K, pts[i], nullptr)) {
      row[i >> 6] |= 1ull << (i & 63);
      count++;
    }
  return count;
}

// The three launches of orbfe_pnp_solve on one problem.  hyps[H], words[H][ceil(n / 64)], refines[H], refine_words[H][..], diag[H],
// refine_diag[H] (the last two may be null), result, result_mask[ceil(n / 64)].  A set that is not a draw gives an all-zero record
// (refine -1) and row, as the device form does; rows without a refine stay zero.
extern "C" void pnp_host_solve(const orbfe_pnp_camera* camera, const orbfe_pnp_point* pts, int n, const int32_t* sets, int H, int min_inliers,
                               orbfe_pnp_hypothesis* hyps, uint64_t* words, orbfe_pnp_refine* refines, uint64_t* refine_words,
                               orbfe_pnp_diag* diag, orbfe_pnp_diag* refine_diag, orbfe_pnp_result* result, uint64_t* result_mask) {
  const int n_words = (n + 63) / 64;
  memset(hyps, 0, (size_t)H * sizeof(*hyps));
  memset(words, 0, (size_t)H * n_words * 8);
  memset(refines, 0, (size_t)H * sizeof(*refines));
  memset(refine_words, 0, (size_t)H * n_words * 8);
  if (diag) memset(diag, 0, (size_t)H * sizeof(*diag));
  if (refine_diag) memset(refine_diag, 0, (size_t)H * sizeof(*refine_diag));
  memset(result, 0, sizeof(*result));
  memset(result_mask, 0, (size_t)n_words * 8);
  result->returned = result->best = -1;
  if (n < 4 || n < min_inliers) return;
  PnpCamera K;
  K.fu = camera->fx; K.fv = camera->fy; K.uc = camera->cx; K.vc = camera->cy;
  std::vector<PnpWork> work(1);
  PnpWork& w = work[0];
  for (int h = 0; h < H; h++) {   // pnp_hypotheses_kernel
    hyps[h].refine = -1;
    const int32_t* s = sets + 4 * h;
    if (!pnp_set_ok(s[0], s[1], s[2], s[3], n)) continue;
    const int winner = pnp_compute_pose(&w, K, pts, s, 4, 0, 1);
    memcpy(hyps[h].R, w.st[winner].R, sizeof(hyps[h].R));
    memcpy(hyps[h].t, w.st[winner].t, sizeof(hyps[h].t));
    hyps[h].winner = winner;
    hyps[h].n_inliers = check_inliers(w, winner, K, pts, n, words + (size_t)h * n_words);
    if (diag) pnp_fill_diag(&w, diag + h);
  }
  std::vector<int32_t> sel((size_t)n);
  int prev = 0;
  for (int h = 0; h < H; h++) {   // pnp_refine_kernel
    const int c = hyps[h].n_inliers;
    const bool is_best = c >= min_inliers && c >= 4 && c > prev;
    prev = c > prev ? c : prev;
    if (!is_best) continue;
    int m = 0;
    for (int i = 0; i < n; i++)
      if ((words[(size_t)h * n_words + (i >> 6)] >> (i & 63)) & 1) sel[m++] = i;
    const int winner = pnp_compute_pose(&w, K, pts, sel.data(), m, 0, 1);
    orbfe_pnp_refine& r = refines[h];
    memcpy(r.R, w.st[winner].R, sizeof(r.R));
    memcpy(r.t, w.st[winner].t, sizeof(r.t));
    r.winner = winner; r.n_used = m;
    r.n_inliers = check_inliers(w, winner, K, pts, n, refine_words + (size_t)h * n_words);
    r.success = r.n_inliers > min_inliers;
    hyps[h].refine = h;
    if (refine_diag) pnp_fill_diag(&w, refine_diag + h);
  }
  int returned = -1, best = -1;   // pnp_select_kernel
  for (int h = 0; h < H; h++) {
    if (hyps[h].refine != h) continue;
    best = h;
    if (refines[h].success) { returned = h; break; }
  }
  const bool refined = returned >= 0;
  if (!refined) returned = best;
  result->returned = returned; result->refined = refined; result->best = best;
  if (best < 0) return;
  result->best_inliers = hyps[best].n_inliers;
  const double* R = refined ? refines[best].R : hyps[best].R;
  const double* t = refined ? refines[best].t : hyps[best].t;
  result->n_inliers = refined ? refines[best].n_inliers : hyps[best].n_inliers;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) result->Tcw[4 * i + j] = (float)R[3 * i + j];
    result->Tcw[4 * i + 3] = (float)t[i];
  }
  memcpy(result_mask, (refined ? refine_words : words) + (size_t)best * n_words, (size_t)n_words * 8);
}
