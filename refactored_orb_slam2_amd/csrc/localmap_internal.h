// localmap_internal.h -- the reading of Tracking::UpdateLocalKeyFrames behind its vote, Tracking::UpdateLocalPoints and the skip flag
// of Tracking::SearchLocalPoints, once, for the kernel (localmap_kernels.hip) and for host code that wants the same answers
// (tests/cpp_localmap/host_arith.cpp).  __host__ __device__ inline functions; everything is integer.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   Tracking::UpdateLocalKeyFrames   L/src/Tracking.cc:1161-1214 (the expansion; the vote :1115-1159 is covis_internal.h's)
//   Tracking::UpdateLocalPoints      L/src/Tracking.cc:1090-1113
//   Tracking::SearchLocalPoints      L/src/Tracking.cc:1036-1049, :1057-1060 (mnLastFrameSeen, also set at :711 and :825)
//
// mnTrackReferenceForFrame == mCurrentFrame.mnId is one mark bit per keyframe row and one per point; mnLastFrameSeen ==
// mCurrentFrame.mnId is a second bit per point, set for the frame's own good slots and the also-seen slice.  The expansion loops over
// the VOTED entries only (itEndKF is taken before the loop, :1163-1164) and the `break` at :1206 leaves that loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbfe.h"

#define LM_HD __host__ __device__ __forceinline__
#define LM_THREADS 1024                          // threads of the kernel's workgroup: one round of the union
#define LM_LIST_MAX (ORBFE_COV_MAX_CONN + 3)     // rows a list can hold: max(n_voted, 80 + 3)
#define LM_RECORD_DWORDS 18                      // sizeof(orbfe_map_point) / 4
#define LM_SKIP_DWORD 8                          // offsetof(orbfe_map_point, skip) / 4

struct LmTables {
  const orbfe_lm_graph* graph; const int32_t* children; int n_children_total;
  const orbfe_cov_keyframe* kfs; const uint8_t* kf_bad; int n_kf;
  const uint8_t* point_bad; int n_points;
  const int32_t* slots; int n_slots_total;
  const int32_t* seen; int n_seen_total;
};

LM_HD bool lm_row_ok(int32_t r, int n) { return r >= 0 && r < n; }
LM_HD bool lm_slice_ok(int32_t offset, int32_t n, int total) { return n >= 0 && offset >= 0 && offset <= total - n; }
LM_HD bool lm_slot_ok(int32_t p, int n_points) { return p >= -1 && p < n_points; }
LM_HD bool lm_bit(const uint32_t* bits, int32_t i) { return (bits[i >> 5] >> (i & 31)) & 1u; }
LM_HD uint32_t lm_mask(int32_t i) { return 1u << (i & 31); }

// the vote header: 0 go on, else the status the frame ends with
LM_HD int lm_vote_status(const orbfe_cov_header& V, int conn_cap, int n_kf) {
  if (V.status == ORBFE_COV_EMPTY) return ORBFE_LM_EMPTY;
  if (V.status != ORBFE_COV_OK || V.n_written < 0 || V.n_written > conn_cap || V.kf_max < -1 || V.kf_max >= n_kf) return ORBFE_LM_REFUSED;
  return ORBFE_LM_OK;
}
// a local keyframe's slot array may be walked
LM_HD bool lm_keyframe_ok(const orbfe_cov_keyframe& K) { return K.n_keys == 0 || (K.n_keys > 0 && K.slots && !(K.slots & 3)); }
// :1178-1179 and :1192-1193: a neighbour or a child is taken when it is not bad and not marked
LM_HD bool lm_eligible(const uint8_t* kf_bad, const uint32_t* marked, int32_t r) { return !kf_bad[r] && !lm_bit(marked, r); }
LM_HD bool lm_size_stops(int size) { return size > ORBFE_LM_SIZE; }   // :1167

template <class V>
LM_HD const V* lm_at(uint64_t address) { return reinterpret_cast<const V*>((uintptr_t)address); }

LM_HD void lm_header_set(orbfe_lm_header& H, int n_voted, int n_kf, int n_points, int ref_kf, int stop, int status) {
  H.n_voted = n_voted; H.n_local_kf = n_kf; H.n_local_points = n_points; H.ref_kf = ref_kf; H.stop = stop; H.status = status;
  H.reserved[0] = H.reserved[1] = 0;
}

// The expansion for one frame, sequentially.  list: LM_LIST_MAX rows; marked: (n_kf + 31) / 32 words, zeroed by the caller.  Returns
// the list's length, or -1: the frame is refused.
LM_HD int lm_expand_sequential(const LmTables& T, const orbfe_cov_entry* E, int n_voted, int32_t* list, uint32_t* marked, int& stop) {
  for (int i = 0; i < n_voted; i++) {
    const int32_t k = E[i].kf;
    if (!lm_row_ok(k, T.n_kf)) return -1;
    list[i] = k;
    marked[k >> 5] |= lm_mask(k);
  }
  int size = n_voted;
  stop = ORBFE_LM_STOP_EXHAUSTED;
  for (int i = 0; i < n_voted; i++) {
    if (lm_size_stops(size)) { stop = ORBFE_LM_STOP_SIZE; break; }
    const orbfe_lm_graph& G = T.graph[list[i]];
    if (G.n_best < 0 || G.n_best > ORBFE_LM_BEST || !lm_slice_ok(G.child_offset, G.n_children, T.n_children_total) || G.parent < -1 ||
        G.parent >= T.n_kf)
      return -1;
    for (int j = 0; j < G.n_best; j++)   // every one is checked, taken or not: what the lanes of the kernel do
      if (!lm_row_ok(G.best[j], T.n_kf)) return -1;
    for (int j = 0; j < G.n_best; j++)
      if (lm_eligible(T.kf_bad, marked, G.best[j])) {
        list[size++] = G.best[j];
        marked[G.best[j] >> 5] |= lm_mask(G.best[j]);
        break;
      }
    for (int c0 = 0; c0 < G.n_children; c0 += 64) {   // in chunks of 64, each checked whole before one of it is taken
      const int n = G.n_children - c0 < 64 ? G.n_children - c0 : 64;
      for (int j = 0; j < n; j++)
        if (!lm_row_ok(T.children[G.child_offset + c0 + j], T.n_kf)) return -1;
      int j = 0;
      while (j < n && !lm_eligible(T.kf_bad, marked, T.children[G.child_offset + c0 + j])) j++;
      if (j < n) {
        const int32_t c = T.children[G.child_offset + c0 + j];
        list[size++] = c;
        marked[c >> 5] |= lm_mask(c);
        break;
      }
    }
    if (G.parent >= 0 && !lm_bit(marked, G.parent)) {   // :1202-1207: badness not tested, and the outer loop ends
      list[size++] = G.parent;
      marked[G.parent >> 5] |= lm_mask(G.parent);
      stop = ORBFE_LM_STOP_PARENT;
      break;
    }
  }
  return size;
}

// Everything of one frame that must hold before a byte of it but the header is written: the local keyframes' slot arrays, the
// frame's slots and its also-seen slice.
LM_HD bool lm_validate_sequential(const LmTables& T, const int32_t* list, int n_local, const orbfe_cov_subject& S, const orbfe_lm_frame* F) {
  for (int j = 0; j < n_local; j++) {
    const orbfe_cov_keyframe& K = T.kfs[list[j]];
    if (!lm_keyframe_ok(K)) return false;
    for (int i = 0; i < K.n_keys; i++)
      if (!lm_slot_ok(lm_at<int32_t>(K.slots)[i], T.n_points)) return false;
  }
  for (int i = 0; i < S.n_slots; i++)
    if (!lm_slot_ok(T.slots[S.slot_offset + i], T.n_points)) return false;
  if (F) {
    if (!lm_slice_ok(F->seen_offset, F->n_seen, T.n_seen_total)) return false;
    for (int i = 0; i < F->n_seen; i++)
      if (!lm_row_ok(T.seen[F->seen_offset + i], T.n_points)) return false;
  }
  return true;
}

// The whole reading for one frame, sequentially: what the kernel spreads over a workgroup.  list: LM_LIST_MAX rows; kf_marked:
// (n_kf + 31) / 32 words and p_marked: (n_points + 31) / 32 words, zeroed by the caller.  local_kf [kf_cap], local_points [p_cap],
// map_points [p_cap] (with records; both may be null), n_points_out: this frame's.
LM_HD void lm_local_map_sequential(const LmTables& T, const orbfe_cov_header& V, const orbfe_cov_entry* E, int conn_cap,
                                   const orbfe_cov_subject& S, const orbfe_lm_frame* F, const orbfe_map_point* records, int kf_cap, int p_cap,
                                   int32_t* list, uint32_t* kf_marked, uint32_t* p_marked, orbfe_lm_header& H, int32_t* local_kf,
                                   int32_t* local_points, int32_t* n_points_out, orbfe_map_point* map_points) {
  const int vote = lm_vote_status(V, conn_cap, T.n_kf);
  if (vote == ORBFE_LM_EMPTY) { lm_header_set(H, 0, 0, 0, -1, 0, ORBFE_LM_EMPTY); return; }
  lm_header_set(H, 0, 0, 0, -1, 0, ORBFE_LM_REFUSED);
  *n_points_out = 0;
  if (vote != ORBFE_LM_OK || !lm_slice_ok(S.slot_offset, S.n_slots, T.n_slots_total)) return;
  int stop = 0;
  const int n_local = lm_expand_sequential(T, E, V.n_written, list, kf_marked, stop);
  if (n_local < 0 || !lm_validate_sequential(T, list, n_local, S, F)) return;
  for (int j = 0; j < n_local && j < kf_cap; j++) local_kf[j] = list[j];
  int n = 0;
  for (int j = 0; j < n_local; j++) {
    const orbfe_cov_keyframe& K = T.kfs[list[j]];
    for (int i = 0; i < K.n_keys; i++) {
      const int32_t p = lm_at<int32_t>(K.slots)[i];
      if (p < 0 || lm_bit(p_marked, p) || T.point_bad[p]) continue;
      p_marked[p >> 5] |= lm_mask(p);
      if (n < p_cap) local_points[n] = p;
      n++;
    }
  }
  const int n_write = n < p_cap ? n : p_cap;
  *n_points_out = n_write;
  if (records && map_points) {
    for (int w = 0; w < (T.n_points + 31) / 32; w++) p_marked[w] = 0u;   // now: mnLastFrameSeen == mCurrentFrame.mnId
    for (int i = 0; i < S.n_slots; i++) {
      const int32_t p = T.slots[S.slot_offset + i];
      if (p >= 0 && !T.point_bad[p]) p_marked[p >> 5] |= lm_mask(p);
    }
    if (F)
      for (int i = 0; i < F->n_seen; i++) p_marked[T.seen[F->seen_offset + i] >> 5] |= lm_mask(T.seen[F->seen_offset + i]);
    for (int e = 0; e < n_write; e++) {
      map_points[e] = records[local_points[e]];
      map_points[e].skip = lm_bit(p_marked, local_points[e]) ? 1 : 0;
    }
  }
  lm_header_set(H, V.n_written, n_local, n, V.kf_max, stop, (n_local > kf_cap || n > p_cap) ? ORBFE_LM_OVERFLOW : ORBFE_LM_OK);
}

// ---- launcher (localmap_kernels.hip)
struct LmLaunch {
  LmTables T;
  const orbfe_cov_header* votes; const orbfe_cov_entry* entries; int conn_cap;
  const orbfe_cov_subject* subjects; const orbfe_lm_frame* frames; int S;
  const orbfe_map_point* records;
  int kf_cap, p_cap;
  orbfe_lm_header* headers; int32_t* local_kf; int32_t* local_points; int32_t* n_points_out; orbfe_map_point* map_points;
};
// not hipSuccess: the dynamic LDS limit of the kernel could not be raised on the current device, and nothing was launched
hipError_t orbfe_launch_local_map(const LmLaunch& L, hipStream_t s);
