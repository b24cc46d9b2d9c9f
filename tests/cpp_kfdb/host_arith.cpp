// host_arith.cpp -- csrc/kfdb_internal.h compiled for the HOST: the ordered sum, the minCommonWords rule and the accumulation that
// kfdb_kernels.hip spreads over waves and lanes, so that the arithmetic the kernels execute can be compared with the yardstick on a
// machine without a GPU (tests/test_kfdb_cpu.py).  Same flags as the library (-ffp-contract=off).
#include "../../refactored_orb_slam2_amd/csrc/kfdb_internal.h"

extern "C" int kfdb_host_min_common_words(int max_common_words) { return kfdb_min_common_words(max_common_words); }

extern "C" float kfdb_host_score(const int32_t* q_ids, const double* q_vals, int nq, const int32_t* e_ids, const double* e_vals, int ne) {
  return kfdb_score_ordered(q_ids, q_vals, nq, e_ids, e_vals, ne);
}

// the terms as a wave of the score pass adds them: 64 at a time, each chunk's in lane order
extern "C" float kfdb_host_finish_terms(const double* terms, int n) {
  double sum = 0.0;
  for (int base = 0; base < n; base += 64)
    for (int i = base; i < n && i < base + 64; i++) sum += terms[i];
  return kfdb_l1_finish(sum);
}

extern "C" double kfdb_host_term(double vi, double wi) { return kfdb_l1_term(vi, wi); }

// one entry of lScoreAndMatch with its n counted neighbours: accScore and the slot of pBestKF
extern "C" void kfdb_host_accumulate(float si, int slot, int n, const float* s2, const int32_t* slot2, float* acc, int32_t* best_slot) {
  KfdbAcc a;
  kfdb_acc_start(a, si, slot);
  for (int k = 0; k < n; k++) kfdb_acc_neighbour(a, s2[k], slot2[k]);
  *acc = a.acc;
  *best_slot = a.best_slot;
}

extern "C" float kfdb_host_min_score_to_retain(float best_acc_score) { return kfdb_min_score_to_retain(best_acc_score); }
extern "C" int kfdb_host_strip(void) { return KFDB_STRIP; }
