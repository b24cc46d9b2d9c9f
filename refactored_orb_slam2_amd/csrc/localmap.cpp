// localmap.cpp -- C ABI of the local map of a tracked frame (include/orbfe.h: orbfe_local_map*): Tracking::UpdateLocalKeyFrames behind
// its vote, Tracking::UpdateLocalPoints and the skip flag of Tracking::SearchLocalPoints.  The entry points validate, stage and launch
// localmap_kernels.hip.  No CPU fallback: without a device both are an error.
#include <string.h>

#include "host_internal.h"
#include "localmap_internal.h"

namespace {

struct LmCounts {
  int S, conn_cap, n_children_total, n_kf, n_points, n_slots_total, n_seen_total, kf_cap, p_cap;
};

bool counts_ok(const char* where, const LmCounts& c) {
  if (c.S < 0 || c.S > ORBFE_LM_MAX_FRAMES || c.conn_cap < 1 || c.conn_cap > ORBFE_COV_MAX_CONN || c.kf_cap < 1 ||
      c.kf_cap > ORBFE_LM_MAX_KF_CAP || c.p_cap < 1 || c.p_cap > ORBFE_LM_MAX_P_CAP) {
    orbfe_set_error("%s: S %d (0 .. %d), conn_cap %d (1 .. %d), kf_cap %d (1 .. %d), p_cap %d (1 .. %d)", where, c.S, ORBFE_LM_MAX_FRAMES,
                    c.conn_cap, ORBFE_COV_MAX_CONN, c.kf_cap, ORBFE_LM_MAX_KF_CAP, c.p_cap, ORBFE_LM_MAX_P_CAP);
    return false;
  }
  if (c.n_kf < 0 || c.n_kf > ORBFE_LM_MAX_KEYFRAMES || c.n_points < 0 || c.n_points > ORBFE_LM_MAX_POINTS || c.n_children_total < 0 ||
      c.n_children_total > ORBFE_LM_MAX_TOTAL_CHILDREN || c.n_slots_total < 0 || c.n_slots_total > ORBFE_LM_MAX_TOTAL_SLOTS ||
      c.n_seen_total < 0 || c.n_seen_total > ORBFE_LM_MAX_TOTAL_SEEN) {
    orbfe_set_error("%s: n_kf %d (0 .. %d), n_points %d (0 .. %d), n_children_total %d (0 .. %d), n_slots_total %d (0 .. %d), n_seen_total "
                    "%d (0 .. %d)", where, c.n_kf, ORBFE_LM_MAX_KEYFRAMES, c.n_points, ORBFE_LM_MAX_POINTS, c.n_children_total,
                    ORBFE_LM_MAX_TOTAL_CHILDREN, c.n_slots_total, ORBFE_LM_MAX_TOTAL_SLOTS, c.n_seen_total, ORBFE_LM_MAX_TOTAL_SEEN);
    return false;
  }
  return true;
}

// what both forms require of their pointers; the names are those of the device form
bool pointers_ok(const char* where, const LmCounts& c, const void* headers, const void* entries, const void* graph, const void* children,
                 const void* keyframes, const void* kf_bad, const void* point_bad, const void* slots, const void* subjects,
                 const void* frames, const void* seen, const void* records, const void* lm_headers, const void* local_kf,
                 const void* local_points, const void* n_points_out, const void* map_points) {
  if ((c.S > 0 && (!headers || !entries || !subjects || !lm_headers || !local_kf || !local_points || !n_points_out)) ||
      (c.n_kf > 0 && (!graph || !keyframes || !kf_bad)) || (c.n_children_total > 0 && !children) || (c.n_points > 0 && !point_bad) ||
      (c.n_slots_total > 0 && !slots) || (c.n_seen_total > 0 && (!seen || !frames)) || (c.S > 0 && records && !map_points)) {
    orbfe_set_error("%s: the vote, the subjects and the outputs are required for S > 0, every table for a count > 0, the also-seen array "
                    "with its frame records, map_points with point_records", where);
    return false;
  }
  return true;
}

bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" int orbfe_local_map_batch_device(int S, const orbfe_cov_header* d_headers, const orbfe_cov_entry* d_entries, int conn_cap,
                                            const orbfe_lm_graph* d_graph, const int32_t* d_children, int n_children_total,
                                            const orbfe_cov_keyframe* d_keyframes, const uint8_t* d_kf_bad, int n_kf,
                                            const uint8_t* d_point_bad, int n_points, const int32_t* d_slots, int n_slots_total,
                                            const orbfe_cov_subject* d_subjects, const orbfe_lm_frame* d_frames, const int32_t* d_seen,
                                            int n_seen_total, const orbfe_map_point* d_point_records, int kf_cap, int p_cap,
                                            orbfe_lm_header* d_lm_headers, int32_t* d_local_kf, int32_t* d_local_points, int32_t* d_n_points,
                                            orbfe_map_point* d_map_points, void* stream) {
  const char* where = "local map batch";
  const LmCounts c = {S, conn_cap, n_children_total, n_kf, n_points, n_slots_total, n_seen_total, kf_cap, p_cap};
  if (!counts_ok(where, c)) return ORBFE_ERR_INVALID;
  if (!pointers_ok(where, c, d_headers, d_entries, d_graph, d_children, d_keyframes, d_kf_bad, d_point_bad, d_slots, d_subjects, d_frames,
                   d_seen, d_point_records, d_lm_headers, d_local_kf, d_local_points, d_n_points, d_map_points))
    return ORBFE_ERR_INVALID;
  if (misaligned(d_headers, 3) || misaligned(d_entries, 3) || misaligned(d_graph, 3) || misaligned(d_children, 3) ||
      misaligned(d_keyframes, 7) || misaligned(d_slots, 3) || misaligned(d_subjects, 3) || misaligned(d_frames, 3) || misaligned(d_seen, 3) ||
      misaligned(d_point_records, 3) || misaligned(d_lm_headers, 3) || misaligned(d_local_kf, 3) || misaligned(d_local_points, 3) ||
      misaligned(d_n_points, 3) || misaligned(d_map_points, 3)) {
    orbfe_set_error("%s: records must be 4-byte aligned, the keyframe table 8-byte", where);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (S == 0) return ORBFE_OK;
  LmLaunch L;
  memset(&L, 0, sizeof(L));
  L.T.graph = d_graph; L.T.children = d_children; L.T.n_children_total = n_children_total; L.T.kfs = d_keyframes; L.T.kf_bad = d_kf_bad;
  L.T.n_kf = n_kf; L.T.point_bad = d_point_bad; L.T.n_points = n_points; L.T.slots = d_slots; L.T.n_slots_total = n_slots_total;
  L.T.seen = d_seen; L.T.n_seen_total = n_seen_total;
  L.votes = d_headers; L.entries = d_entries; L.conn_cap = conn_cap; L.subjects = d_subjects; L.frames = d_frames; L.S = S;
  L.records = d_point_records; L.kf_cap = kf_cap; L.p_cap = p_cap;
  L.headers = d_lm_headers; L.local_kf = d_local_kf; L.local_points = d_local_points; L.n_points_out = d_n_points; L.map_points = d_map_points;
  const hipError_t lds = orbfe_launch_local_map(L, (hipStream_t)stream);
  if (lds != hipSuccess) return hip_status("local map batch: raising the kernel's dynamic LDS limit failed", lds);
  return hip_status("local map batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_local_map(const orbfe_cov_header* headers, const orbfe_cov_entry* entries, int conn_cap, const orbfe_lm_graph* graph,
                               const int32_t* children, int n_children_total, const orbfe_cov_keyframe* keyframes, const uint8_t* kf_bad,
                               int n_kf, const uint8_t* point_bad, int n_points, const int32_t* slots, int n_slots_total,
                               const orbfe_cov_subject* subjects, const orbfe_lm_frame* frames, const int32_t* seen, int n_seen_total,
                               const orbfe_map_point* point_records, int S, int kf_cap, int p_cap, orbfe_lm_header* lm_headers,
                               int32_t* local_kf, int32_t* local_points, int32_t* n_points_out, orbfe_map_point* map_points) {
  const char* where = "local map";
  const LmCounts c = {S, conn_cap, n_children_total, n_kf, n_points, n_slots_total, n_seen_total, kf_cap, p_cap};
  if (!counts_ok(where, c)) return ORBFE_ERR_INVALID;
  if (!pointers_ok(where, c, headers, entries, graph, children, keyframes, kf_bad, point_bad, slots, subjects, frames, seen, point_records,
                   lm_headers, local_kf, local_points, n_points_out, map_points))
    return ORBFE_ERR_INVALID;
  if ((size_t)S * (size_t)p_cap > ORBFE_LM_MAX_TOTAL_RECORDS) {
    orbfe_set_error("%s: S x p_cap = %d x %d records (at most %d)", where, S, p_cap, ORBFE_LM_MAX_TOTAL_RECORDS);
    return ORBFE_ERR_INVALID;
  }
  if (S == 0) return have_device() ? ORBFE_OK : ORBFE_ERR_NO_DEVICE;   // nothing behind the counts is read
  size_t n_keys_total = 0;
  for (int k = 0; k < n_kf; k++) {
    const orbfe_cov_keyframe& K = keyframes[k];
    if (K.n_keys < 0 || K.n_keys > ORBFE_COV_MAX_KEYS) {
      orbfe_set_error("%s: keyframe %d has n_keys %d (0 .. %d)", where, k, K.n_keys, ORBFE_COV_MAX_KEYS);
      return ORBFE_ERR_INVALID;
    }
    if (K.slots) n_keys_total += (size_t)K.n_keys;
  }
  if (n_keys_total > ORBFE_COV_MAX_TOTAL_KEYS) {
    orbfe_set_error("%s: the table holds %zu slots in all (at most %d)", where, n_keys_total, ORBFE_COV_MAX_TOTAL_KEYS);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;

  HostCall h(where);
  const size_t b_vote = (size_t)S * sizeof(orbfe_cov_header), b_ent = (size_t)S * conn_cap * sizeof(orbfe_cov_entry),
               b_graph = (size_t)n_kf * sizeof(orbfe_lm_graph), b_child = (size_t)n_children_total * 4,
               b_kf = (size_t)n_kf * sizeof(orbfe_cov_keyframe), b_slots = (size_t)n_slots_total * 4, b_sub = (size_t)S * sizeof(orbfe_cov_subject),
               b_frames = frames ? (size_t)S * sizeof(orbfe_lm_frame) : 0, b_seen = (size_t)n_seen_total * 4,
               b_rec = point_records ? (size_t)n_points * sizeof(orbfe_map_point) : 0;
  const size_t o_vote = h.in(b_vote), o_ent = h.in(b_ent), o_graph = h.in(b_graph), o_child = h.in(b_child), o_kf = h.in(b_kf),
               o_kbad = h.in((size_t)n_kf), o_pbad = h.in((size_t)n_points), o_slots = h.in(b_slots), o_sub = h.in(b_sub),
               o_frames = h.in(b_frames), o_seen = h.in(b_seen), o_rec = h.in(b_rec), o_keys = h.in(n_keys_total * 4);
  // the output group: what is short first, so that one copy of its head covers what a caller without records needs
  const size_t o_head = h.out((size_t)S * sizeof(orbfe_lm_header)), o_np = h.out((size_t)S * 4), o_lkf = h.out((size_t)S * kf_cap * 4),
               o_lp = h.out((size_t)S * p_cap * 4), o_mp = h.out(point_records ? (size_t)S * p_cap * sizeof(orbfe_map_point) : 0);
  int rc;
  if ((rc = h.open())) return rc;
  uint8_t *const hp = h.host(0), *const d = h.dev(0);
  memcpy(hp + o_vote, headers, b_vote);
  memcpy(hp + o_ent, entries, b_ent);
  memcpy(hp + o_sub, subjects, b_sub);
  if (n_kf) { memcpy(hp + o_graph, graph, b_graph); memcpy(hp + o_kbad, kf_bad, (size_t)n_kf); }
  if (b_child) memcpy(hp + o_child, children, b_child);
  if (n_points) memcpy(hp + o_pbad, point_bad, (size_t)n_points);
  if (b_slots) memcpy(hp + o_slots, slots, b_slots);
  if (b_frames) memcpy(hp + o_frames, frames, b_frames);
  if (b_seen) memcpy(hp + o_seen, seen, b_seen);
  if (b_rec) memcpy(hp + o_rec, point_records, b_rec);
  orbfe_cov_keyframe* table = (orbfe_cov_keyframe*)(hp + o_kf);
  size_t at = 0;
  for (int k = 0; k < n_kf; k++) {   // only `slots` and `n_keys` are read: the other addresses are not staged and read as null
    const orbfe_cov_keyframe& K = keyframes[k];
    table[k] = K;
    table[k].keys_un = table[k].u_right = table[k].depth = 0;
    if (K.slots && K.n_keys) {
      memcpy(hp + o_keys + at * 4, lm_at<uint8_t>(K.slots), (size_t)K.n_keys * 4);
      table[k].slots = (uint64_t)(uintptr_t)(d + o_keys + at * 4);
      at += (size_t)K.n_keys;
    }
  }
  if ((rc = h.upload())) return rc;
  LmLaunch L;
  memset(&L, 0, sizeof(L));
  L.T.graph = (const orbfe_lm_graph*)(d + o_graph); L.T.children = (const int32_t*)(d + o_child); L.T.n_children_total = n_children_total;
  L.T.kfs = (const orbfe_cov_keyframe*)(d + o_kf); L.T.kf_bad = d + o_kbad; L.T.n_kf = n_kf; L.T.point_bad = d + o_pbad; L.T.n_points = n_points;
  L.T.slots = (const int32_t*)(d + o_slots); L.T.n_slots_total = n_slots_total; L.T.seen = (const int32_t*)(d + o_seen);
  L.T.n_seen_total = n_seen_total;
  L.votes = (const orbfe_cov_header*)(d + o_vote); L.entries = (const orbfe_cov_entry*)(d + o_ent); L.conn_cap = conn_cap;
  L.subjects = (const orbfe_cov_subject*)(d + o_sub); L.frames = frames ? (const orbfe_lm_frame*)(d + o_frames) : nullptr; L.S = S;
  L.records = point_records ? (const orbfe_map_point*)(d + o_rec) : nullptr; L.kf_cap = kf_cap; L.p_cap = p_cap;
  L.headers = (orbfe_lm_header*)(d + o_head); L.local_kf = (int32_t*)(d + o_lkf); L.local_points = (int32_t*)(d + o_lp);
  L.n_points_out = (int32_t*)(d + o_np); L.map_points = (orbfe_map_point*)(d + o_mp);
  const hipError_t lds = orbfe_launch_local_map(L, h.stream);
  if (lds != hipSuccess) return hip_status("local map: raising the kernel's dynamic LDS limit failed", lds);
  if ((rc = h.finish(h.out_bytes()))) return rc;
  const orbfe_lm_header* rh = (const orbfe_lm_header*)(hp + o_head);
  for (int s = 0; s < S; s++) {   // the header, and the heads that were written: what lies behind them stays the caller's
    lm_headers[s] = rh[s];
    if (rh[s].status == ORBFE_LM_EMPTY) continue;
    const int np = ((const int32_t*)(hp + o_np))[s];
    n_points_out[s] = np;
    if (rh[s].status == ORBFE_LM_REFUSED) continue;
    const int nk = rh[s].n_local_kf < kf_cap ? rh[s].n_local_kf : kf_cap;
    if (nk > 0) memcpy(local_kf + (size_t)s * kf_cap, hp + o_lkf + (size_t)s * kf_cap * 4, (size_t)nk * 4);
    if (np > 0 && np <= p_cap) {
      memcpy(local_points + (size_t)s * p_cap, hp + o_lp + (size_t)s * p_cap * 4, (size_t)np * 4);
      if (point_records)
        memcpy(map_points + (size_t)s * p_cap, hp + o_mp + (size_t)s * p_cap * sizeof(orbfe_map_point), (size_t)np * sizeof(orbfe_map_point));
    }
  }
  return ORBFE_OK;
}
