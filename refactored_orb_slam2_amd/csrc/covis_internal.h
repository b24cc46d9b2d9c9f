// covis_internal.h -- the reading of KeyFrame::UpdateConnections, the vote of Tracking::UpdateLocalKeyFrames and
// LocalMapping::KeyFrameCulling, once, for the kernels (covis_kernels.hip) and for host code that wants the same answers
// (tests/cpp_covis/host_arith.cpp).  __host__ __device__ inline functions; everything is integer but two comparisons.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   KeyFrame::UpdateConnections      L/src/KeyFrame.cc:268-354
//   Tracking::UpdateLocalKeyFrames   L/src/Tracking.cc:1115-1159 (the vote)
//   LocalMapping::KeyFrameCulling    L/src/LocalMapping.cc:595-655, with KeyFrame::SetBadFlag L/src/KeyFrame.cc:416-434 and
//                                    MapPoint::EraseObservation L/src/MapPoint.cc:112-136
//
// Counts.  The counter is a histogram over keyframe rows.  What the reference does with its std::map afterwards is an ordering of the
// rows with a counter > 0, and both orders are the DESCENDING order of one 64-bit key (kf_order values are distinct, so keys are):
//   CONNECTIONS  weight << 32 | order      sort(vPairs) ascending on pair<int, KeyFrame*>, then push_front of each: descending
//   VOTES        0xffffffff - order        the iteration of the map: ascending order
// pKFmax is the first row in ascending order with the strict maximum (`mit->second > nmax`): the greatest weight << 32 |
// (0xffffffff - order).  An entry that does not exist has key 0; every real key is > 0 (weight >= 1, order < 32 768).
//
// Culling.  The reference mutates the map between two local keyframes; here the set of rows culled so far (one bit per row) stands
// for the mutation, and a point's state follows from its list (cov_cull_slot).  Equal to the mutation because Observations() only
// falls: a point is bad after some erase exactly when it is after the last one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbfe.h"

#define COV_HD __host__ __device__ __forceinline__
#define COV_THREADS 256   // threads of both kernels' workgroups

struct CovTables {
  const orbfe_mp_obs* obs; int n_obs_total;
  const orbfe_mp_point* points; const uint8_t* point_bad; const int32_t* n_obs_weighted; int n_points;
  const int32_t* kf_order; const uint8_t* kf_bad;   // counts
  const orbfe_cov_keyframe* kfs;                    // culling
  int n_kf;
};

COV_HD uint64_t cov_key_connections(uint32_t w, int32_t order) { return ((uint64_t)w << 32) | (uint32_t)order; }
COV_HD uint64_t cov_key_votes(int32_t order) { return (uint64_t)(0xffffffffu - (uint32_t)order); }
COV_HD uint64_t cov_key_max(uint32_t w, int32_t order) { return ((uint64_t)w << 32) | (0xffffffffu - (uint32_t)order); }
// the sort key of row r with counter w; 0: the row has no entry
COV_HD uint64_t cov_entry_key(int mode, uint32_t w, int32_t order, bool kf_bad) {
  if (w == 0) return 0;
  if (mode == ORBFE_COV_CONNECTIONS) return cov_key_connections(w, order);
  return kf_bad ? 0 : cov_key_votes(order);
}
COV_HD bool cov_ordered(uint32_t w) { return w >= ORBFE_COV_TH; }   // `mit->second >= th`

COV_HD bool cov_subject_ok(const orbfe_cov_subject& S, int n_slots_total, int n_kf) {
  if (S.mode != ORBFE_COV_CONNECTIONS && S.mode != ORBFE_COV_VOTES) return false;
  if (S.n_slots < 0 || S.slot_offset < 0 || S.slot_offset > n_slots_total - S.n_slots) return false;
  return S.mode == ORBFE_COV_VOTES || (S.self >= -1 && S.self < n_kf);
}
COV_HD bool cov_list_ok(const orbfe_mp_point& Q, int n_obs_total) {
  return Q.n_obs >= 0 && Q.obs_offset >= 0 && Q.obs_offset <= n_obs_total - Q.n_obs;
}
COV_HD bool cov_row_ok(int32_t kf, int n_kf) { return kf >= 0 && kf < n_kf; }

// One slot of a subject.  bump(row) adds 1 to that row's counter.  false: the subject is refused.
template <class Bump>
COV_HD bool cov_count_slot(const CovTables& T, int32_t p, int32_t self, Bump bump) {
  if (p == -1) return true;
  if (p < -1 || p >= T.n_points) return false;
  if (T.point_bad[p]) return true;
  const orbfe_mp_point Q = T.points[p];
  if (!cov_list_ok(Q, T.n_obs_total)) return false;
  for (int j = 0; j < Q.n_obs; j++) {
    const int32_t kf = T.obs[Q.obs_offset + j].kf;
    if (!cov_row_ok(kf, T.n_kf) || !cov_row_ok(T.kf_order[kf], T.n_kf)) return false;
    if (kf != self) bump(kf);
  }
  return true;
}

COV_HD void cov_header_refused(orbfe_cov_header& H) {
  H.n_counted = H.n_ordered = 0; H.kf_max = -1; H.w_max = 0; H.status = ORBFE_COV_REFUSED; H.n_written = H.single = H.reserved = 0;
}

// The whole reading for one subject, sequentially: what the count kernel spreads over a workgroup.  counter: n_kf words, zeroed by
// the caller.  Entries are picked greatest key first, one scan of the counters each.
COV_HD void cov_count_sequential(const CovTables& T, const int32_t* slots, int n_slots_total, const orbfe_cov_subject& S, int conn_cap,
                                 uint32_t* counter, orbfe_cov_header& H, orbfe_cov_entry* E) {
  cov_header_refused(H);
  if (!cov_subject_ok(S, n_slots_total, T.n_kf)) return;
  const int32_t self = S.mode == ORBFE_COV_VOTES ? -1 : S.self;
  for (int i = 0; i < S.n_slots; i++)
    if (!cov_count_slot(T, slots[S.slot_offset + i], self, [counter](int32_t kf) { counter[kf]++; })) return;
  int n_counted = 0, n_ordered = 0, n_entries = 0, kf_max = -1;
  uint64_t best = 0;
  for (int r = 0; r < T.n_kf; r++) {
    const uint32_t w = counter[r];
    if (!w) continue;
    n_counted++;
    const uint64_t key = cov_entry_key(S.mode, w, T.kf_order[r], T.kf_bad[r] != 0);
    if (!key) continue;
    n_entries++;
    if (S.mode == ORBFE_COV_VOTES || cov_ordered(w)) n_ordered++;
    const uint64_t m = cov_key_max(w, T.kf_order[r]);
    if (m > best) { best = m; kf_max = r; }
  }
  H.n_counted = n_counted; H.n_ordered = n_ordered; H.kf_max = kf_max; H.w_max = (int32_t)(best >> 32);
  H.n_written = n_entries < conn_cap ? n_entries : conn_cap;
  H.single = S.mode == ORBFE_COV_CONNECTIONS && n_ordered == 0 && n_counted > 0;
  H.status = n_counted == 0 ? ORBFE_COV_EMPTY : n_entries > conn_cap ? ORBFE_COV_OVERFLOW : ORBFE_COV_OK;
  uint64_t below = ~(uint64_t)0;
  for (int e = 0; e < H.n_written; e++) {
    uint64_t pick = 0;
    int row = -1;
    for (int r = 0; r < T.n_kf; r++) {
      const uint64_t key = cov_entry_key(S.mode, counter[r], T.kf_order[r], T.kf_bad[r] != 0);
      if (key > pick && key < below) { pick = key; row = r; }
    }
    if (row < 0) { H.n_written = e; break; }   // equal keys: orders that are not distinct, outside the stated domain
    E[e].kf = row; E[e].weight = (int32_t)counter[row];
    below = pick;
  }
}

// ---- culling
COV_HD bool cov_depth_gate(float depth, float th_depth) { return depth > th_depth || depth < 0; }          // LocalMapping.cc:620
COV_HD bool cov_octave_counts(int32_t octave_i, int32_t octave) { return octave_i <= octave + 1; }           // :638
COV_HD int cov_erase_weight(float u_right) { return u_right >= 0 ? 2 : 1; }                                  // MapPoint.cc:118-121
COV_HD bool cov_point_bad(int n_obs_weighted, int removed) { return removed > 0 && n_obs_weighted - removed <= 2; }   // MapPoint.cc:129
COV_HD bool cov_redundant(int n_redundant, int n_mps) { return (double)n_redundant > 0.9 * (double)n_mps; }  // LocalMapping.cc:652
COV_HD bool cov_culled(const uint32_t* culled, int32_t row) { return (culled[row >> 5] >> (row & 31)) & 1u; }

// what the row itself must satisfy before a slot of it is read
COV_HD bool cov_keyframe_ok(const orbfe_cov_keyframe& K, int monocular) {
  if (K.n_keys < 0) return false;
  if (K.n_keys == 0) return true;   // nothing behind its addresses is read
  if (!K.slots || !K.keys_un || (!monocular && !K.depth)) return false;
  return !((K.keys_un | K.u_right | K.depth | K.slots) & 3);
}

template <class V>
COV_HD const V* cov_at(uint64_t address) { return reinterpret_cast<const V*>((uintptr_t)address); }

// Slot i of local row k (K = kfs[k], accepted by cov_keyframe_ok): bit 0 = it counts to nMPs, bit 1 = it is redundant; -1 = the row
// is refused.  culled: one bit per row, the rows culled before k.
COV_HD int cov_cull_slot(const CovTables& T, const uint32_t* culled, int32_t k, const orbfe_cov_keyframe& K, int i, int monocular) {
  const int32_t p = cov_at<int32_t>(K.slots)[i];
  if (p == -1) return 0;
  if (p < -1 || p >= T.n_points) return -1;
  if (T.point_bad[p]) return 0;
  const orbfe_mp_point Q = T.points[p];
  if (!cov_list_ok(Q, T.n_obs_total)) return -1;
  const int32_t octave = cov_at<orbfe_keypoint>(K.keys_un)[i].octave;
  int removed = 0, n_obs = 0;
  for (int j = 0; j < Q.n_obs; j++) {
    const orbfe_mp_obs o = T.obs[Q.obs_offset + j];
    if (!cov_row_ok(o.kf, T.n_kf)) return -1;
    const orbfe_cov_keyframe* Ko = T.kfs + o.kf;
    if (o.idx < 0 || o.idx >= Ko->n_keys) return -1;
    if (cov_culled(culled, o.kf)) {
      const uint64_t ur = Ko->u_right;
      if (ur & 3) return -1;
      removed += ur ? cov_erase_weight(cov_at<float>(ur)[o.idx]) : 1;
    } else if (o.kf != k) {
      const uint64_t keys = Ko->keys_un;
      if (!keys || (keys & 3)) return -1;
      if (n_obs < 3 && cov_octave_counts(cov_at<orbfe_keypoint>(keys)[o.idx].octave, octave)) n_obs++;
    }
  }
  const int nw = T.n_obs_weighted[p];
  if (cov_point_bad(nw, removed)) return 0;
  if (!monocular && cov_depth_gate(cov_at<float>(K.depth)[i], K.th_depth)) return 0;
  return (nw - removed > 3 && n_obs >= 3) ? 3 : 1;
}

COV_HD int cov_verdict(int n_redundant, int n_mps, int flags) {
  if (!cov_redundant(n_redundant, n_mps)) return ORBFE_COV_KEPT;
  return (flags & ORBFE_COV_NOT_ERASE) ? ORBFE_COV_MARKED : ORBFE_COV_CULLED;
}
COV_HD bool cov_problem_ok(const orbfe_cov_problem& P, int n_local_total) {
  return P.n_local >= 0 && P.local_offset >= 0 && P.local_offset <= n_local_total - P.n_local;
}

// The whole reading for one problem, sequentially.  culled: (n_kf + 31) / 32 words, zeroed by the caller.
COV_HD void cov_cull_sequential(const CovTables& T, const int32_t* local, int n_local_total, const orbfe_cov_problem& P, uint32_t* culled,
                                orbfe_cov_verdict* V) {
  if (!cov_problem_ok(P, n_local_total)) return;
  for (int j = 0; j < P.n_local; j++) {
    const int32_t k = local[P.local_offset + j];
    orbfe_cov_verdict& R = V[P.local_offset + j];
    R.n_mps = R.n_redundant = R.reserved = 0;
    R.verdict = ORBFE_COV_ROW_REFUSED;
    if (!cov_row_ok(k, T.n_kf)) continue;
    const orbfe_cov_keyframe K = T.kfs[k];
    if (K.flags & ORBFE_COV_IS_ID0) { R.verdict = ORBFE_COV_SKIPPED_ID0; continue; }
    if (!cov_keyframe_ok(K, P.monocular)) continue;
    int n_mps = 0, n_red = 0;
    bool ok = true;
    for (int i = 0; ok && i < K.n_keys; i++) {
      const int r = cov_cull_slot(T, culled, k, K, i, P.monocular);
      if (r < 0) ok = false; else { n_mps += r & 1; n_red += r >> 1; }
    }
    if (!ok) continue;
    R.n_mps = n_mps; R.n_redundant = n_red;
    R.verdict = cov_verdict(n_red, n_mps, K.flags);
    if (R.verdict == ORBFE_COV_CULLED) culled[k >> 5] |= 1u << (k & 31);
  }
}

// ---- launchers (covis_kernels.hip)
struct CovCountLaunch {
  CovTables T;
  const int32_t* slots; int n_slots_total;
  const orbfe_cov_subject* subjects; int S;
  int conn_cap;
  orbfe_cov_header* headers; orbfe_cov_entry* entries;
};
struct CovCullLaunch {
  CovTables T;
  const int32_t* local; int n_local_total;
  const orbfe_cov_problem* problems; int Q;
  orbfe_cov_verdict* verdicts;
};
// not hipSuccess: the dynamic LDS limit of the count kernel could not be raised on the current device, and nothing was launched
hipError_t orbfe_launch_covis_count(const CovCountLaunch& L, hipStream_t s);
void orbfe_launch_covis_cull(const CovCullLaunch& L, hipStream_t s);
