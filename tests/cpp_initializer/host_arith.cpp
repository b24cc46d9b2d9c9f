// host_arith.cpp -- csrc/initializer_internal.h compiled for the HOST: the loops that initializer_kernels.hip spreads over
// workgroups, waves and lanes, in the same orders (a lane's score terms in match order, the 64 lane sums in one butterfly; the rows
// of [A; V] as array elements), so that the arithmetic the kernels execute can be compared with the numpy yardstick on a machine
// without a GPU (tests/test_initializer_cpu.py) and with the device byte for byte (tests/test_initializer_gpu.py).  Same flags as
// the library (-ffp-contract=off).  Single-threaded.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/initializer_internal.h"

static float butterfly64(float* x) {
  float z[64];
  for (int d = 32; d > 0; d >>= 1) {
    for (int i = 0; i < 64; i++) z[i] = x[i] + x[i ^ d];
    memcpy(x, z, sizeof(z));
  }
  return x[0];
}

// The outputs of orbfe_initializer_initialize with every optional one: hyps [2][H] and words [2][H][ceil(n1 / 64)] (model H first),
// cands [8].  Returns 0, or -1 for an input the C ABI refuses.
extern "C" int init_host_run(const orbfe_init_params* par, const float* keys1, int n1, const float* keys2, int n2, const int32_t* matches12,
                             const int32_t* sets, int H, orbfe_init_result* result, float* P3D, uint64_t* tri, uint64_t* inl,
                             orbfe_init_hypothesis* hyps, uint64_t* words, orbfe_init_candidate* cands) {
  const size_t n1_words = ((size_t)n1 + 63) / 64;
  std::vector<float> mxy;
  std::vector<int> mi1;
  for (int i = 0; i < n1; i++) {
    const int m = matches12[i];
    if (m >= n2) return -1;
    if (m < 0) continue;
    mxy.insert(mxy.end(), {keys1[2 * i], keys1[2 * i + 1], keys2[2 * m], keys2[2 * m + 1]});
    mi1.push_back(i);
  }
  const int N = (int)mi1.size(), n_words = (N + 63) / 64;
  orbfe_init_result& r = *result;
  memset(&r, 0, sizeof(r));
  r.best_h = r.best_f = r.best_candidate = -1;
  r.n_matches = N;
  memset(P3D, 0, (size_t)n1 * 12);
  memset(tri, 0, n1_words * 8);
  memset(inl, 0, n1_words * 8);
  memset(hyps, 0, (size_t)2 * H * sizeof(*hyps));
  memset(words, 0, (size_t)2 * H * n1_words * 8);
  memset(cands, 0, 8 * sizeof(*cands));
  if (N < 8) {
    r.reason = ORBFE_INIT_FEW_MATCHES;
    return 0;
  }
  // prologue
  IniNorm N1, N2;
  ini_normalize(keys1, n1, N1);
  ini_normalize(keys2, n2, N2);
  float T1[9], T2[9], T2inv[9], T2t[9], K[9];
  ini_norm_matrix(N1, T1);
  ini_norm_matrix(N2, T2);
  ini_inv33(T2, T2inv);
  ini_transpose33(T2, T2t);
  ini_K(*par, K);
  r.norm1[0] = N1.mx; r.norm1[1] = N1.my; r.norm1[2] = N1.sx; r.norm1[3] = N1.sy;
  r.norm2[0] = N2.mx; r.norm2[1] = N2.my; r.norm2[2] = N2.sx; r.norm2[3] = N2.sy;
  const float invSigmaSquare = ini_inv_sigma_square(par->sigma);
  // hypotheses
  float best_score[2] = {0.0f, 0.0f};
  int best[2] = {-1, -1};
  for (int model = 0; model < 2; model++)
    for (int h = 0; h < H; h++) {
      const int32_t* set = sets + (size_t)h * 8;
      orbfe_init_hypothesis& R = hyps[(size_t)model * H + h];
      uint64_t* row = words + ((size_t)model * H + h) * n1_words;
      if (!ini_set_ok(set, N)) continue;
      IniRow rows[25];
      for (int l = 0; l < 25; l++) rows[l] = ini_row_v(l - 16);
      for (int l = 0; l < (model == 0 ? 16 : 8); l++) {
        const float* m = &mxy[4 * (size_t)set[model == 0 ? l >> 1 : l]];
        const float u1 = ini_norm_x(N1, m[0]), v1 = ini_norm_y(N1, m[1]), u2 = ini_norm_x(N2, m[2]), v2 = ini_norm_y(N2, m[3]);
        rows[l] = model == 0 ? ini_row_h(l & 1, u1, v1, u2, v2) : ini_row_f(u1, v1, u2, v2);
      }
      float v9[9], M[9], Minv[9] = {0};
      ini_null9_host(rows, v9);
      if (model == 0) ini_model_h(v9, T1, T2inv, M, Minv);
      else ini_model_f(v9, T1, T2t, M);
      float lane_sum[64] = {0};
      int count = 0;
      for (int i = 0; i < N; i++) {
        const float* m = &mxy[4 * (size_t)i];
        float a1, a2;
        const bool ok = model == 0 ? ini_check_h(M, Minv, m[0], m[1], m[2], m[3], invSigmaSquare, a1, a2)
                                   : ini_check_f(M, m[0], m[1], m[2], m[3], invSigmaSquare, a1, a2);
        lane_sum[i & 63] += a1;
        lane_sum[i & 63] += a2;
        if (ok) {
          row[i >> 6] |= 1ull << (i & 63);
          count++;
        }
      }
      memcpy(R.M, M, sizeof(M));
      R.score = butterfly64(lane_sum);
      R.n_inliers = count;
      R.status = 1;
      ini_first_max(R.score, h, best_score[model], best[model]);
    }
  // select
  const float SH = best_score[0], SF = best_score[1];
  const float RH = SH / (SH + SF);
  int model = 0;
  if (best[0] >= 0 || best[1] >= 0) model = (double)RH > 0.40 ? 1 : 2;
  r.best_h = best[0]; r.best_f = best[1]; r.score_h = SH; r.score_f = SF;
  r.rh = model ? RH : 0.0f;
  r.model = model;
  if (best[0] >= 0) memcpy(r.H21, hyps[best[0]].M, sizeof(r.H21));
  if (best[1] >= 0) memcpy(r.F21, hyps[(size_t)H + best[1]].M, sizeof(r.F21));
  if (!model) {
    r.reason = ORBFE_INIT_NO_MODEL;
    return 0;
  }
  const size_t chosen = model == 1 ? (size_t)best[0] : (size_t)H + best[1];
  r.n_inliers = hyps[chosen].n_inliers;
  memcpy(inl, words + chosen * n1_words, (size_t)n_words * 8);
  if (model == 1) {
    if (ini_candidates_h(r.H21, K, cands)) r.n_candidates = 8;
    else r.reason = ORBFE_INIT_H_DEGENERATE;
  } else {
    ini_candidates_f(r.F21, K, cands);
    r.n_candidates = 4;
  }
  // CheckRT
  const float th2 = ini_th2(par->sigma);
  for (int c = 0; c < r.n_candidates; c++) {
    IniPose P;
    ini_pose(K, cands[c].R, cands[c].t, P);
    std::vector<uint32_t> keys;
    for (int i = 0; i < N; i++) {
      if (!((inl[i >> 6] >> (i & 63)) & 1ull)) continue;
      float x[3], cosv;
      if (ini_check_point(*par, K, P, th2, mxy[4 * (size_t)i], mxy[4 * (size_t)i + 1], mxy[4 * (size_t)i + 2], mxy[4 * (size_t)i + 3], x, cosv))
        keys.push_back(ini_cos_key(cosv));
    }
    cands[c].n_good = (int)keys.size();
    if (!keys.empty()) {
      std::sort(keys.begin(), keys.end());
      cands[c].parallax = ini_parallax_degrees(ini_key_cos(keys[std::min<size_t>(50, keys.size() - 1)]));
    }
  }
  // decide
  bool success = false;
  if (r.n_candidates == 8) success = ini_decide_h(cands, r.n_inliers, *par, r);
  else if (r.n_candidates == 4) success = ini_decide_f(cands, r.n_inliers, *par, r);
  r.success = success;
  if (success) {
    const orbfe_init_candidate& w = cands[r.best_candidate];
    IniPose P;
    ini_pose(K, w.R, w.t, P);
    for (int i = 0; i < N; i++) {
      if (!((inl[i >> 6] >> (i & 63)) & 1ull)) continue;
      float x[3], cosv;
      const int code = ini_check_point(*par, K, P, th2, mxy[4 * (size_t)i], mxy[4 * (size_t)i + 1], mxy[4 * (size_t)i + 2], mxy[4 * (size_t)i + 3], x, cosv);
      if (!code) continue;
      const int i1 = mi1[i];
      memcpy(P3D + 3 * (size_t)i1, x, 12);
      if (code == 2) {
        tri[i1 >> 6] |= 1ull << (i1 & 63);
        r.n_triangulated++;
      }
    }
    memcpy(r.R21, w.R, sizeof(r.R21));
    memcpy(r.t21, w.t, sizeof(r.t21));
  }
  return 0;
}

// the acceptance rules alone, on engineered counts: model 1 reads eight (n_good, parallax), model 2 four
extern "C" int init_host_decide(int model, const int32_t* n_good, const float* parallax, int N, const orbfe_init_params* par,
                                orbfe_init_result* result) {
  orbfe_init_candidate c[8];
  memset(c, 0, sizeof(c));
  for (int i = 0; i < (model == 1 ? 8 : 4); i++) {
    c[i].n_good = n_good[i];
    c[i].parallax = parallax[i];
  }
  memset(result, 0, sizeof(*result));
  return model == 1 ? ini_decide_h(c, N, *par, *result) : ini_decide_f(c, N, *par, *result);
}
// the selection rule alone, on engineered scores, in the order of the device's scan: lanes of 64, then the merge
extern "C" int init_host_first_max(const float* scores, int H) {
  float bs[64];
  int b[64];
  for (int l = 0; l < 64; l++) {
    bs[l] = 0.0f;
    b[l] = -1;
    for (int h = l; h < H; h += 64) ini_first_max(scores[h], h, bs[l], b[l]);
  }
  float best_score = 0.0f;
  int best = -1;
  for (int l = 0; l < 64; l++)
    if (b[l] >= 0 && (best < 0 || bs[l] > best_score || (bs[l] == best_score && b[l] < best))) {
      best_score = bs[l];
      best = b[l];
    }
  return best;
}
