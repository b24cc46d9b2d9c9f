// host_arith.cpp -- csrc/mapping_internal.h compiled for the HOST: the loop over the rows that mapping_kernels.hip runs one thread
// each, so that the arithmetic the kernel executes can be compared with the numpy yardstick on a machine without a GPU
// (tests/test_mapping_cpu.py).  Same flags as the library (-ffp-contract=off).
#include <string.h>

#include "../../refactored_orb_slam2_amd/csrc/mapping_internal.h"

extern "C" void mapping_host_triangulate(const orbfe_tri_view* v1, const orbfe_keypoint* k1, const float* ur1, const float* d1, int nA,
                                         const orbfe_tri_view* v2, const orbfe_keypoint* k2, const float* ur2, const float* d2, int nB,
                                         const int32_t* matchA, orbfe_new_point* out) {
  for (int i = 0; i < nA; i++) {
    orbfe_new_point P;
    memset(&P, 0, sizeof(P));
    P.idx2 = -1;
    P.code = ORBFE_TRI_NO_MATCH;
    const int j = matchA[i];
    if (j >= 0 && j < nB && k1[i].octave >= 0 && k1[i].octave < v1->n_levels && k2[j].octave >= 0 && k2[j].octave < v2->n_levels) {
      const TriObs o1{k1[i].x, k1[i].y, ur1 ? ur1[i] : -1.f, ur1 && ur1[i] >= 0 ? d1[i] : -1.f, k1[i].octave};
      const TriObs o2{k2[j].x, k2[j].y, ur2 ? ur2[j] : -1.f, ur2 && ur2[j] >= 0 ? d2[j] : -1.f, k2[j].octave};
      int path;
      P.code = tri_pair(*v1, *v2, o1, o2, v1->level_sigma2[o1.octave], v2->level_sigma2[o2.octave], v1->scale_factors[o1.octave],
                        v2->scale_factors[o2.octave], v1->scale_factors[v1->n_levels - 1], 1.5f * v1->scale_factors[1], P, &path);
      P.path = path;
      P.idx2 = j;
      if (P.code != ORBFE_TRI_OK) memset(&P, 0, 32);
    }
    out[i] = P;
  }
}
