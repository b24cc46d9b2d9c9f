// host_arith.cpp -- csrc/covis_internal.h compiled for the HOST: the counting, the sort keys, the header rules, the culled-set reading
// of KeyFrameCulling and every check that covis_kernels.hip spreads over lanes, so that what the kernels evaluate can be compared with
// the yardstick on a machine without a GPU (tests/test_covis_cpu.py).  Same signatures as the host forms of include/orbfe.h.
#include <string.h>

#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/covis_internal.h"

extern "C" void covis_host_count(const orbfe_mp_obs* obs, int n_obs_total, const orbfe_mp_point* points, const uint8_t* point_bad, int n_points,
                                 const int32_t* kf_order, const uint8_t* kf_bad, int n_kf, const int32_t* slots, int n_slots_total,
                                 const orbfe_cov_subject* subjects, int S, int conn_cap, orbfe_cov_header* headers, orbfe_cov_entry* entries) {
  CovTables T;
  memset(&T, 0, sizeof(T));
  T.obs = obs; T.n_obs_total = n_obs_total; T.points = points; T.point_bad = point_bad; T.n_points = n_points;
  T.kf_order = kf_order; T.kf_bad = kf_bad; T.n_kf = n_kf;
  std::vector<uint32_t> counter;
  for (int s = 0; s < S; s++) {
    counter.assign((size_t)n_kf + 1, 0u);
    cov_count_sequential(T, slots, n_slots_total, subjects[s], conn_cap, counter.data(), headers[s], entries + (size_t)s * conn_cap);
  }
}

extern "C" void covis_host_cull(const orbfe_mp_obs* obs, int n_obs_total, const orbfe_mp_point* points, const uint8_t* point_bad,
                                const int32_t* n_obs_weighted, int n_points, const orbfe_cov_keyframe* keyframes, int n_kf,
                                const int32_t* local, int n_local_total, const orbfe_cov_problem* problems, int Q, orbfe_cov_verdict* verdicts) {
  CovTables T;
  memset(&T, 0, sizeof(T));
  T.obs = obs; T.n_obs_total = n_obs_total; T.points = points; T.point_bad = point_bad; T.n_obs_weighted = n_obs_weighted;
  T.n_points = n_points; T.kfs = keyframes; T.n_kf = n_kf;
  std::vector<uint32_t> culled;
  for (int q = 0; q < Q; q++) {
    culled.assign((size_t)(n_kf + 31) / 32 + 1, 0u);
    cov_cull_sequential(T, local, n_local_total, problems[q], culled.data(), verdicts);
  }
}

extern "C" int covis_host_redundant(int n_redundant, int n_mps) { return cov_redundant(n_redundant, n_mps) ? 1 : 0; }
extern "C" int covis_host_threads(void) { return COV_THREADS; }
