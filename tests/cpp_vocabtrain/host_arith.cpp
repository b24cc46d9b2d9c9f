// host_arith.cpp -- csrc/vocab_train_internal.h compiled for the HOST: the draw, the first-centre index, the cut with its retry on a
// draw of 0, the pick with its fall-through to the last index, the majority threshold and the Hamming distance that
// vocab_train_kernels.hip evaluates, so that they can be compared with the yardstick on a machine without a GPU
// (tests/test_vocab_train_cpu.py).  Same flags as the library (-ffp-contract=off).
#include "../../refactored_orb_slam2_amd/csrc/vocab_train_internal.h"

extern "C" uint32_t vt_host_draw(uint64_t seed, uint32_t level, uint64_t path, uint32_t j) { return vt_draw(seed, level, path, j); }
extern "C" int vt_host_first_index(uint32_t r, int n) { return vt_first_index(r, n); }
extern "C" double vt_host_cut(uint32_t r, int64_t dist_sum) { return vt_cut(r, dist_sum); }
extern "C" int64_t vt_host_cut_target(double cut) { return vt_cut_target(cut); }
extern "C" int vt_host_pick(const int32_t* min_dists, int n, double cut) { return vt_pick(min_dists, n, cut); }
extern "C" int vt_host_majority(int n) { return vt_majority(n); }
extern "C" int vt_host_hamming(const uint8_t* a, const uint8_t* b) {
  uint32_t x[8], y[8];
  __builtin_memcpy(x, a, 32);
  __builtin_memcpy(y, b, 32);
  return vt_hamming(x, y);
}

// the header's retry rule, vt_cut_retry, on a given sequence of draws instead of the generator's (a draw of 0 has probability 2^-31
// there); *used = draws consumed.  The sequence must hold a draw that is not 0.
struct ArrayDraws {
  const uint32_t* draws;
  int* used;
  uint32_t operator()() { return draws[(*used)++]; }
};
extern "C" double vt_host_cut_retry(const uint32_t* draws, int64_t dist_sum, int* used) {
  *used = 0;
  ArrayDraws source{draws, used};
  return vt_cut_retry(source, dist_sum);
}
// the same through the generator: the cut and the counter after it
extern "C" double vt_host_cut_draw(uint64_t seed, uint32_t level, uint64_t path, uint32_t* j, int64_t dist_sum) {
  return vt_cut_draw(seed, level, path, j, dist_sum);
}
extern "C" int vt_host_chunk(void) { return VT_CHUNK; }
