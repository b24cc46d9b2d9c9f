// covis.cpp -- C ABI of the covisibility graph (include/orbfe.h: orbfe_covis_*): the counts of KeyFrame::UpdateConnections and of the
// vote of Tracking::UpdateLocalKeyFrames, and LocalMapping::KeyFrameCulling.  The entry points validate, stage and launch
// covis_kernels.hip.  No CPU fallback: without a device all four are an error.
#include <string.h>

#include "covis_internal.h"
#include "host_internal.h"

namespace {

// the map tables both operations read
bool tables_ok(const char* where, int n_obs_total, int n_points, int n_kf) {
  if (n_obs_total < 0 || n_obs_total > ORBFE_COV_MAX_TOTAL_OBS || n_points < 0 || n_points > ORBFE_COV_MAX_POINTS || n_kf < 0 ||
      n_kf > ORBFE_COV_MAX_KEYFRAMES) {
    orbfe_set_error("%s: n_obs_total %d (0 .. %d), n_points %d (0 .. %d), n_kf %d (0 .. %d)", where, n_obs_total, ORBFE_COV_MAX_TOTAL_OBS,
                    n_points, ORBFE_COV_MAX_POINTS, n_kf, ORBFE_COV_MAX_KEYFRAMES);
    return false;
  }
  return true;
}

bool count_counts_ok(const char* where, int S, int n_obs_total, int n_points, int n_kf, int n_slots_total, int conn_cap) {
  if (!tables_ok(where, n_obs_total, n_points, n_kf)) return false;
  if (S < 0 || S > ORBFE_COV_MAX_SUBJECTS || n_slots_total < 0 || n_slots_total > ORBFE_COV_MAX_TOTAL_SLOTS || conn_cap < 1 ||
      conn_cap > ORBFE_COV_MAX_CONN) {
    orbfe_set_error("%s: S %d (0 .. %d), n_slots_total %d (0 .. %d), conn_cap %d (1 .. %d)", where, S, ORBFE_COV_MAX_SUBJECTS, n_slots_total,
                    ORBFE_COV_MAX_TOTAL_SLOTS, conn_cap, ORBFE_COV_MAX_CONN);
    return false;
  }
  return true;
}

bool cull_counts_ok(const char* where, int Q, int n_obs_total, int n_points, int n_kf, int n_local_total) {
  if (!tables_ok(where, n_obs_total, n_points, n_kf)) return false;
  if (Q < 0 || Q > ORBFE_COV_MAX_PROBLEMS || n_local_total < 0 || n_local_total > ORBFE_COV_MAX_TOTAL_LOCAL) {
    orbfe_set_error("%s: Q %d (0 .. %d), n_local_total %d (0 .. %d)", where, Q, ORBFE_COV_MAX_PROBLEMS, n_local_total,
                    ORBFE_COV_MAX_TOTAL_LOCAL);
    return false;
  }
  return true;
}

bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" int orbfe_covis_count_batch_device(int S, const orbfe_mp_obs* d_obs, int n_obs_total, const orbfe_mp_point* d_points,
                                              const uint8_t* d_point_bad, int n_points, const int32_t* d_kf_order, const uint8_t* d_kf_bad,
                                              int n_kf, const int32_t* d_slots, int n_slots_total, const orbfe_cov_subject* d_subjects,
                                              int conn_cap, orbfe_cov_header* d_headers, orbfe_cov_entry* d_entries, void* stream) {
  const char* where = "covisibility counts batch";
  if (!count_counts_ok(where, S, n_obs_total, n_points, n_kf, n_slots_total, conn_cap)) return ORBFE_ERR_INVALID;
  if ((S > 0 && (!d_subjects || !d_headers || !d_entries)) || (n_obs_total > 0 && !d_obs) || (n_points > 0 && (!d_points || !d_point_bad)) ||
      (n_kf > 0 && (!d_kf_order || !d_kf_bad)) || (n_slots_total > 0 && !d_slots)) {
    orbfe_set_error("%s: subjects, headers and entries are required for S > 0, every table for a count > 0", where);
    return ORBFE_ERR_INVALID;
  }
  if (misaligned(d_obs, 3) || misaligned(d_points, 3) || misaligned(d_kf_order, 3) || misaligned(d_slots, 3) || misaligned(d_subjects, 3) ||
      misaligned(d_headers, 3) || misaligned(d_entries, 3)) {
    orbfe_set_error("%s: records must be 4-byte aligned", where);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (S == 0) return ORBFE_OK;
  CovCountLaunch L;
  memset(&L, 0, sizeof(L));
  L.T.obs = d_obs; L.T.n_obs_total = n_obs_total; L.T.points = d_points; L.T.point_bad = d_point_bad; L.T.n_points = n_points;
  L.T.kf_order = d_kf_order; L.T.kf_bad = d_kf_bad; L.T.n_kf = n_kf;
  L.slots = d_slots; L.n_slots_total = n_slots_total; L.subjects = d_subjects; L.S = S; L.conn_cap = conn_cap;
  L.headers = d_headers; L.entries = d_entries;
  const hipError_t lds = orbfe_launch_covis_count(L, (hipStream_t)stream);
  if (lds != hipSuccess) return hip_status("covisibility counts batch: raising the count kernel's dynamic LDS limit failed", lds);
  return hip_status("covisibility counts batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_covis_count(const orbfe_mp_obs* obs, int n_obs_total, const orbfe_mp_point* points, const uint8_t* point_bad,
                                 int n_points, const int32_t* kf_order, const uint8_t* kf_bad, int n_kf, const int32_t* slots,
                                 int n_slots_total, const orbfe_cov_subject* subjects, int S, int conn_cap, orbfe_cov_header* headers,
                                 orbfe_cov_entry* entries) {
  const char* where = "covisibility counts";
  if (!count_counts_ok(where, S, n_obs_total, n_points, n_kf, n_slots_total, conn_cap)) return ORBFE_ERR_INVALID;
  if ((S > 0 && (!subjects || !headers || !entries)) || (n_obs_total > 0 && !obs) || (n_points > 0 && (!points || !point_bad)) ||
      (n_kf > 0 && (!kf_order || !kf_bad)) || (n_slots_total > 0 && !slots)) {
    orbfe_set_error("%s: subjects, headers and entries are required for S > 0, every table for a count > 0", where);
    return ORBFE_ERR_INVALID;
  }
  if ((size_t)S * (size_t)conn_cap > ORBFE_COV_MAX_TOTAL_ENTRIES) {
    orbfe_set_error("%s: S x conn_cap = %d x %d entries (at most %d)", where, S, conn_cap, ORBFE_COV_MAX_TOTAL_ENTRIES);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (S == 0) return ORBFE_OK;   // nothing behind the counts is read

  HostCall c(where);
  const size_t b_obs = (size_t)n_obs_total * sizeof(orbfe_mp_obs), b_pts = (size_t)n_points * sizeof(orbfe_mp_point),
               b_order = (size_t)n_kf * 4, b_slots = (size_t)n_slots_total * 4, b_sub = (size_t)S * sizeof(orbfe_cov_subject);
  const size_t o_obs = c.in(b_obs), o_pts = c.in(b_pts), o_pbad = c.in((size_t)n_points), o_order = c.in(b_order), o_kbad = c.in((size_t)n_kf),
               o_slots = c.in(b_slots), o_sub = c.in(b_sub);
  const size_t o_head = c.out((size_t)S * sizeof(orbfe_cov_header)), o_ent = c.out((size_t)S * conn_cap * sizeof(orbfe_cov_entry));
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  if (b_obs) memcpy(h + o_obs, obs, b_obs);
  if (b_pts) { memcpy(h + o_pts, points, b_pts); memcpy(h + o_pbad, point_bad, (size_t)n_points); }
  if (n_kf) { memcpy(h + o_order, kf_order, b_order); memcpy(h + o_kbad, kf_bad, (size_t)n_kf); }
  if (b_slots) memcpy(h + o_slots, slots, b_slots);
  memcpy(h + o_sub, subjects, b_sub);
  if ((rc = c.upload())) return rc;
  CovCountLaunch L;
  memset(&L, 0, sizeof(L));
  L.T.obs = (const orbfe_mp_obs*)(d + o_obs); L.T.n_obs_total = n_obs_total; L.T.points = (const orbfe_mp_point*)(d + o_pts);
  L.T.point_bad = d + o_pbad; L.T.n_points = n_points; L.T.kf_order = (const int32_t*)(d + o_order); L.T.kf_bad = d + o_kbad; L.T.n_kf = n_kf;
  L.slots = (const int32_t*)(d + o_slots); L.n_slots_total = n_slots_total; L.subjects = (const orbfe_cov_subject*)(d + o_sub); L.S = S;
  L.conn_cap = conn_cap; L.headers = (orbfe_cov_header*)(d + o_head); L.entries = (orbfe_cov_entry*)(d + o_ent);
  const hipError_t lds = orbfe_launch_covis_count(L, c.stream);
  if (lds != hipSuccess) return hip_status("covisibility counts: raising the count kernel's dynamic LDS limit failed", lds);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  const orbfe_cov_header* rh = (const orbfe_cov_header*)(h + o_head);
  const orbfe_cov_entry* re = (const orbfe_cov_entry*)(h + o_ent);
  for (int s = 0; s < S; s++) {   // the header, and the entries that were written: what lies behind them stays the caller's
    headers[s] = rh[s];
    const int n = rh[s].n_written < 0 ? 0 : rh[s].n_written > conn_cap ? conn_cap : rh[s].n_written;
    if (n) memcpy(entries + (size_t)s * conn_cap, re + (size_t)s * conn_cap, (size_t)n * sizeof(orbfe_cov_entry));
  }
  return ORBFE_OK;
}

extern "C" int orbfe_covis_cull_keyframes_batch_device(int Q, const orbfe_mp_obs* d_obs, int n_obs_total, const orbfe_mp_point* d_points,
                                                       const uint8_t* d_point_bad, const int32_t* d_n_obs_weighted, int n_points,
                                                       const orbfe_cov_keyframe* d_keyframes, int n_kf, const int32_t* d_local,
                                                       int n_local_total, const orbfe_cov_problem* d_problems, orbfe_cov_verdict* d_verdicts,
                                                       void* stream) {
  const char* where = "keyframe culling batch";
  if (!cull_counts_ok(where, Q, n_obs_total, n_points, n_kf, n_local_total)) return ORBFE_ERR_INVALID;
  if ((Q > 0 && !d_problems) || (n_obs_total > 0 && !d_obs) || (n_points > 0 && (!d_points || !d_point_bad || !d_n_obs_weighted)) ||
      (n_kf > 0 && !d_keyframes) || (n_local_total > 0 && (!d_local || !d_verdicts))) {
    orbfe_set_error("%s: problems are required for Q > 0, every table for a count > 0", where);
    return ORBFE_ERR_INVALID;
  }
  if (misaligned(d_obs, 3) || misaligned(d_points, 3) || misaligned(d_n_obs_weighted, 3) || misaligned(d_keyframes, 7) ||
      misaligned(d_local, 3) || misaligned(d_problems, 3) || misaligned(d_verdicts, 3)) {
    orbfe_set_error("%s: records must be 4-byte aligned, the keyframe table 8-byte", where);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (Q == 0) return ORBFE_OK;
  CovCullLaunch L;
  memset(&L, 0, sizeof(L));
  L.T.obs = d_obs; L.T.n_obs_total = n_obs_total; L.T.points = d_points; L.T.point_bad = d_point_bad; L.T.n_obs_weighted = d_n_obs_weighted;
  L.T.n_points = n_points; L.T.kfs = d_keyframes; L.T.n_kf = n_kf;
  L.local = d_local; L.n_local_total = n_local_total; L.problems = d_problems; L.Q = Q; L.verdicts = d_verdicts;
  orbfe_launch_covis_cull(L, (hipStream_t)stream);
  return hip_status("keyframe culling batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_covis_cull_keyframes(const orbfe_mp_obs* obs, int n_obs_total, const orbfe_mp_point* points, const uint8_t* point_bad,
                                          const int32_t* n_obs_weighted, int n_points, const orbfe_cov_keyframe* keyframes, int n_kf,
                                          const int32_t* local, int n_local_total, const orbfe_cov_problem* problems, int Q,
                                          orbfe_cov_verdict* verdicts) {
  const char* where = "keyframe culling";
  if (!cull_counts_ok(where, Q, n_obs_total, n_points, n_kf, n_local_total)) return ORBFE_ERR_INVALID;
  if ((Q > 0 && !problems) || (n_obs_total > 0 && !obs) || (n_points > 0 && (!points || !point_bad || !n_obs_weighted)) ||
      (n_kf > 0 && !keyframes) || (n_local_total > 0 && (!local || !verdicts))) {
    orbfe_set_error("%s: problems are required for Q > 0, every table for a count > 0", where);
    return ORBFE_ERR_INVALID;
  }
  if (Q == 0) return have_device() ? ORBFE_OK : ORBFE_ERR_NO_DEVICE;   // nothing behind the counts is read
  size_t n_keys_total = 0;
  for (int k = 0; k < n_kf; k++) {
    const orbfe_cov_keyframe& K = keyframes[k];
    if (K.n_keys < 0 || K.n_keys > ORBFE_COV_MAX_KEYS || (K.n_keys > 0 && !K.keys_un)) {
      orbfe_set_error("%s: keyframe %d has n_keys %d (0 .. %d)%s", where, k, K.n_keys, ORBFE_COV_MAX_KEYS,
                      K.n_keys > 0 && K.n_keys <= ORBFE_COV_MAX_KEYS ? " and no keypoint array" : "");
      return ORBFE_ERR_INVALID;
    }
    n_keys_total += (size_t)K.n_keys;
  }
  if (n_keys_total > ORBFE_COV_MAX_TOTAL_KEYS) {
    orbfe_set_error("%s: the table holds %zu keypoints in all (at most %d)", where, n_keys_total, ORBFE_COV_MAX_TOTAL_KEYS);
    return ORBFE_ERR_INVALID;
  }
  for (int q = 0; q < Q; q++)
    if (!cov_problem_ok(problems[q], n_local_total)) {
      orbfe_set_error("%s: problem %d names local keyframes %d .. +%d of %d", where, q, problems[q].local_offset, problems[q].n_local,
                      n_local_total);
      return ORBFE_ERR_INVALID;
    }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;

  HostCall c(where);
  const size_t b_obs = (size_t)n_obs_total * sizeof(orbfe_mp_obs), b_pts = (size_t)n_points * sizeof(orbfe_mp_point), b_w = (size_t)n_points * 4,
               b_kf = (size_t)n_kf * sizeof(orbfe_cov_keyframe), b_local = (size_t)n_local_total * 4, b_prob = (size_t)Q * sizeof(orbfe_cov_problem);
  const size_t o_obs = c.in(b_obs), o_pts = c.in(b_pts), o_pbad = c.in((size_t)n_points), o_w = c.in(b_w), o_kf = c.in(b_kf),
               o_local = c.in(b_local), o_prob = c.in(b_prob);
  // every keyframe's arrays, one after the other: keypoints (28 bytes each), then three 4-byte arrays
  const size_t o_keys = c.in(n_keys_total * sizeof(orbfe_keypoint)), o_right = c.in(n_keys_total * 4), o_depth = c.in(n_keys_total * 4),
               o_slot = c.in(n_keys_total * 4);
  const size_t o_out = c.out((size_t)n_local_total * sizeof(orbfe_cov_verdict));
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  if (b_obs) memcpy(h + o_obs, obs, b_obs);
  if (b_pts) { memcpy(h + o_pts, points, b_pts); memcpy(h + o_pbad, point_bad, (size_t)n_points); memcpy(h + o_w, n_obs_weighted, b_w); }
  if (b_local) memcpy(h + o_local, local, b_local);
  memcpy(h + o_prob, problems, b_prob);
  orbfe_cov_keyframe* table = (orbfe_cov_keyframe*)(h + o_kf);
  size_t at = 0;
  for (int k = 0; k < n_kf; k++) {   // the staged table holds the device addresses of the staged arrays; a null array stays null
    const orbfe_cov_keyframe& K = keyframes[k];
    const size_t n = (size_t)K.n_keys;
    table[k] = K;
    if (n) {
      memcpy(h + o_keys + at * sizeof(orbfe_keypoint), cov_at<uint8_t>(K.keys_un), n * sizeof(orbfe_keypoint));
      table[k].keys_un = (uint64_t)(uintptr_t)(d + o_keys + at * sizeof(orbfe_keypoint));
      if (K.slots) {   // only a row that some problem lists needs its slots
        memcpy(h + o_slot + at * 4, cov_at<uint8_t>(K.slots), n * 4);
        table[k].slots = (uint64_t)(uintptr_t)(d + o_slot + at * 4);
      }
      if (K.u_right) {
        memcpy(h + o_right + at * 4, cov_at<uint8_t>(K.u_right), n * 4);
        table[k].u_right = (uint64_t)(uintptr_t)(d + o_right + at * 4);
      }
      if (K.depth) {
        memcpy(h + o_depth + at * 4, cov_at<uint8_t>(K.depth), n * 4);
        table[k].depth = (uint64_t)(uintptr_t)(d + o_depth + at * 4);
      }
    }
    at += n;
  }
  if ((rc = c.upload())) return rc;
  CovCullLaunch L;
  memset(&L, 0, sizeof(L));
  L.T.obs = (const orbfe_mp_obs*)(d + o_obs); L.T.n_obs_total = n_obs_total; L.T.points = (const orbfe_mp_point*)(d + o_pts);
  L.T.point_bad = d + o_pbad; L.T.n_obs_weighted = (const int32_t*)(d + o_w); L.T.n_points = n_points;
  L.T.kfs = (const orbfe_cov_keyframe*)(d + o_kf); L.T.n_kf = n_kf;
  L.local = (const int32_t*)(d + o_local); L.n_local_total = n_local_total; L.problems = (const orbfe_cov_problem*)(d + o_prob); L.Q = Q;
  L.verdicts = (orbfe_cov_verdict*)(d + o_out);
  orbfe_launch_covis_cull(L, c.stream);
  if ((rc = c.finish((size_t)n_local_total * sizeof(orbfe_cov_verdict)))) return rc;
  const orbfe_cov_verdict* r = (const orbfe_cov_verdict*)(h + o_out);
  for (int q = 0; q < Q; q++)   // the verdict of an element no problem names stays the caller's
    if (problems[q].n_local)
      memcpy(verdicts + problems[q].local_offset, r + problems[q].local_offset, (size_t)problems[q].n_local * sizeof(orbfe_cov_verdict));
  return ORBFE_OK;
}
