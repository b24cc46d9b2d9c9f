// host_arith.cpp -- csrc/sim3_internal.h compiled for the HOST: the loops that sim3_kernels.hip spreads over workgroups, waves and
// lanes, so that the arithmetic the kernel executes can be compared with the numpy yardstick on a machine without a GPU
// (tests/test_sim3_cpu.py).  Same flags as the library (-ffp-contract=off).
#include <string.h>

#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/sim3_internal.h"

// hyps[H], words[H][ceil(n / 64)]; a triple that is not a draw gives an all-zero record and row, as the device form does
extern "C" void sim3_host_solve(const orbfe_sim3_view* v1, const orbfe_sim3_view* v2, const orbfe_sim3_pair* pairs, int n,
                                const int32_t* triples, int H, int fix_scale, orbfe_sim3_hypothesis* hyps, uint64_t* words) {
  std::vector<Sim3Prepared> prep((size_t)n);
  for (int i = 0; i < n; i++) sim3_prepare(*v1, *v2, pairs[i], prep[i]);
  const int n_words = (n + 63) / 64;
  for (int h = 0; h < H; h++) {
    orbfe_sim3_hypothesis& R = hyps[h];
    uint64_t* row = words + (size_t)h * n_words;
    memset(&R, 0, sizeof(R));
    memset(row, 0, (size_t)n_words * 8);
    const int i0 = triples[3 * h], i1 = triples[3 * h + 1], i2 = triples[3 * h + 2];
    if (!sim3_triple_ok(i0, i1, i2, n)) continue;
    Sim3Transform T;
    sim3_horn(prep[i0].c1, prep[i1].c1, prep[i2].c1, prep[i0].c2, prep[i1].c2, prep[i2].c2, fix_scale != 0, T);
    R.s = T.s;
    memcpy(R.R, T.R, sizeof(R.R));
    memcpy(R.t, T.t, sizeof(R.t));
    for (int i = 0; i < n; i++)
      if (sim3_is_inlier(*v1, *v2, T.sR, T.t, T.sRinv, T.tinv, prep[i])) {
        row[i >> 6] |= 1ull << (i & 63);
        R.n_inliers++;
      }
  }
}
