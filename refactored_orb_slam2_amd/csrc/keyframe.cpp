// keyframe.cpp -- C ABI of the keyframe decision and the close stereo points of a tracked frame (include/orbfe.h:
// orbfe_keyframe_insertion*): the statistics tail of Tracking::TrackLocalMap, Tracking::NeedNewKeyFrame and the point creation of
// Tracking::CreateNewKeyFrame / UpdateLastFrame / StereoInitialization.  The entry points validate, stage and launch
// keyframe_kernels.hip.  No CPU fallback: without a device both are an error.
#include <string.h>

#include <vector>

#include "host_internal.h"
#include "keyframe_internal.h"

namespace {

bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// what both forms require; the names are those of orbfe_kf_call
int validate(const char* where, const orbfe_kf_call* call, const orbfe_kf_scales* camera) {
  if (!call || !camera) {
    orbfe_set_error("%s: call and camera are required", where);
    return ORBFE_ERR_INVALID;
  }
  const orbfe_kf_call& C = *call;
  if (C.S < 0 || C.S > ORBFE_KF_MAX_FRAMES || C.cap < 1 || C.cap > ORBFE_KF_MAX_CAP || C.new_cap < 1 || C.new_cap > C.cap || C.p_cap < 1 ||
      C.frame_shift < 0) {
    orbfe_set_error("%s: S %d (0 .. %d), cap %d (1 .. %d), new_cap %d (1 .. cap), p_cap %d (>= 1), frame_shift %d (>= 0)", where, C.S,
                    ORBFE_KF_MAX_FRAMES, C.cap, ORBFE_KF_MAX_CAP, C.new_cap, C.p_cap, C.frame_shift);
    return ORBFE_ERR_INVALID;
  }
  if (C.point_stride < 12 || (C.point_stride & 3) || C.observed_offset < -1 || (C.observed_offset >= 0 && (C.observed_offset & 3)) ||
      C.observed_offset > C.point_stride - 4 || C.ref_kf_stride < 4 || (C.ref_kf_stride & 3)) {
    orbfe_set_error("%s: point_stride %d (>= 12, a multiple of 4), observed_offset %d (-1, or a multiple of 4 inside the record), "
                    "ref_kf_stride %d (>= 4, a multiple of 4)", where, C.point_stride, C.observed_offset, C.ref_kf_stride);
    return ORBFE_ERR_INVALID;
  }
  if (C.n_kf < 0 || C.n_kf > ORBFE_COV_MAX_KEYFRAMES || C.n_map_points < 0 || C.n_map_points > ORBFE_COV_MAX_POINTS ||
      camera->n_levels < 1 || camera->n_levels > ORBFE_MAX_LEVELS) {
    orbfe_set_error("%s: n_kf %d (0 .. %d), n_map_points %d (0 .. %d), n_levels %d (1 .. %d)", where, C.n_kf, ORBFE_COV_MAX_KEYFRAMES,
                    C.n_map_points, ORBFE_COV_MAX_POINTS, camera->n_levels, ORBFE_MAX_LEVELS);
    return ORBFE_ERR_INVALID;
  }
  const int all = ORBFE_KF_STATISTICS | ORBFE_KF_DECISION | ORBFE_KF_CREATE;
  if (C.mode < ORBFE_KF_MODE_KEYFRAME || C.mode > ORBFE_KF_MODE_STEREO_INIT || !C.flags || (C.flags & ~all) ||
      ((C.flags & ORBFE_KF_DECISION) && !(C.flags & ORBFE_KF_STATISTICS))) {
    orbfe_set_error("%s: mode %d (0 .. 2), flags %d (a non-empty subset of STATISTICS | DECISION | CREATE, DECISION only with STATISTICS)",
                    where, C.mode, C.flags);
    return ORBFE_ERR_INVALID;
  }
  const bool stats = C.flags & ORBFE_KF_STATISTICS, decide = C.flags & ORBFE_KF_DECISION, create = C.flags & ORBFE_KF_CREATE;
  if ((C.S > 0 && (!C.n || !C.headers || !C.depth || (C.assigned && (!C.points || !C.n_points)) || (stats && !C.decision) ||
                   (decide && !C.ref_kf) || (create && (!C.keys_un || !C.desc || !C.cam || !C.new_points || !C.new_index || !C.n_new)))) ||
      (decide && ((C.n_kf > 0 && !C.keyframes) || (C.n_map_points > 0 && (!C.point_bad || !C.point_observations))))) {
    orbfe_set_error("%s: n, depth and headers are required for S > 0; points and n_points with assigned; decision with STATISTICS; ref_kf "
                    "and every table with a count > 0 with DECISION; keys_un, desc, cam, new_points, new_index and n_new with CREATE", where);
    return ORBFE_ERR_INVALID;
  }
  if (misaligned(C.keys_un, 3) || misaligned(C.desc, 3) || misaligned(C.depth, 3) || misaligned(C.n, 3) || misaligned(C.cam, 3) ||
      misaligned(C.assigned, 3) || misaligned(C.points, 3) || misaligned(C.n_points, 3) || misaligned(C.decision, 7) ||
      misaligned(C.ref_kf, 3) || misaligned(C.keyframes, 7) || misaligned(C.point_observations, 3) || misaligned(C.n_points_base, 3) ||
      misaligned(C.headers, 3) || misaligned(C.new_points, 3) || misaligned(C.new_index, 3) || misaligned(C.n_new, 3) ||
      misaligned(C.depth_selected, 3)) {
    orbfe_set_error("%s: records must be 4-byte aligned, the decision records and the keyframe table 8-byte", where);
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_keyframe_insertion_batch_device(const orbfe_kf_call* call, const orbfe_kf_scales* camera, void* stream) {
  const char* where = "keyframe insertion batch";
  int rc;
  if ((rc = validate(where, call, camera))) return rc;
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (call->S == 0) return ORBFE_OK;
  KfLaunch L;
  L.C = *call;
  L.cam = *camera;
  const hipError_t lds = orbfe_launch_keyframe_insertion(L, (hipStream_t)stream);
  if (lds != hipSuccess) return hip_status("keyframe insertion batch: raising the kernel's dynamic LDS limit failed", lds);
  return hip_status("keyframe insertion batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_keyframe_insertion(const orbfe_kf_call* call, const orbfe_kf_scales* camera) {
  const char* where = "keyframe insertion";
  int rc;
  if ((rc = validate(where, call, camera))) return rc;
  const orbfe_kf_call& C = *call;
  const int S = C.S;
  if ((size_t)S * (size_t)C.cap > ORBFE_KF_MAX_TOTAL_ROWS || (C.assigned && (size_t)S * (size_t)C.p_cap > ORBFE_KF_MAX_TOTAL_ROWS)) {
    orbfe_set_error("%s: S x cap = %d x %d rows and S x p_cap = %d x %d records (at most %d each)", where, S, C.cap, S, C.p_cap,
                    ORBFE_KF_MAX_TOTAL_ROWS);
    return ORBFE_ERR_INVALID;
  }
  if (S == 0) return have_device() ? ORBFE_OK : ORBFE_ERR_NO_DEVICE;   // nothing behind the counts is read
  const bool stats = C.flags & ORBFE_KF_STATISTICS, decide = C.flags & ORBFE_KF_DECISION, create = C.flags & ORBFE_KF_CREATE;
  // the reference rows some frame names: their slot arrays are staged once each
  std::vector<int64_t> staged_at;
  std::vector<int32_t> ref(decide ? S : 0);
  size_t n_keys_total = 0;
  if (decide) {
    staged_at.assign((size_t)C.n_kf, -1);
    for (int f = 0; f < S; f++) {
      const int32_t r = ref[f] = *reinterpret_cast<const int32_t*>((const uint8_t*)C.ref_kf + (size_t)f * C.ref_kf_stride);
      if (r < 0 || r >= C.n_kf || staged_at[r] >= 0) continue;
      const orbfe_cov_keyframe& K = C.keyframes[r];
      if (K.n_keys > ORBFE_COV_MAX_KEYS) {
        orbfe_set_error("%s: keyframe %d has n_keys %d (at most %d)", where, r, K.n_keys, ORBFE_COV_MAX_KEYS);
        return ORBFE_ERR_INVALID;
      }
      if (K.n_keys <= 0 || !K.slots || (K.slots & 3)) continue;   // the device refuses the frame, or there is nothing to walk
      staged_at[r] = (int64_t)n_keys_total;
      n_keys_total += (size_t)K.n_keys;
    }
    if (n_keys_total > ORBFE_COV_MAX_TOTAL_KEYS) {
      orbfe_set_error("%s: the reference rows hold %zu slots in all (at most %d)", where, n_keys_total, ORBFE_COV_MAX_TOTAL_KEYS);
      return ORBFE_ERR_INVALID;
    }
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;

  HostCall h(where);
  const size_t rows = (size_t)S * C.cap, news = (size_t)S * C.new_cap;
  const size_t b_keys = create ? rows * sizeof(orbfe_keypoint) : 0, b_desc = create ? rows * 32 : 0, b_depth = rows * 4, b_n = (size_t)S * 4,
               b_cam = create ? (size_t)S * sizeof(orbfe_unproject_cam) : 0,
               b_points = C.assigned ? (size_t)S * C.p_cap * C.point_stride : 0, b_np = C.assigned ? (size_t)S * 4 : 0,
               b_outl = C.outlier ? rows : 0, b_dec = stats ? (size_t)S * sizeof(orbfe_kf_decision_in) : 0, b_ref = decide ? (size_t)S * 4 : 0,
               b_kf = decide ? (size_t)C.n_kf * sizeof(orbfe_cov_keyframe) : 0, b_pbad = decide ? (size_t)C.n_map_points : 0,
               b_pobs = decide ? (size_t)C.n_map_points * 4 : 0, b_base = (create && C.n_points_base) ? (size_t)S * 4 : 0;
  const size_t o_keys = h.in(b_keys), o_desc = h.in(b_desc), o_depth = h.in(b_depth), o_n = h.in(b_n), o_cam = h.in(b_cam),
               o_points = h.in(b_points), o_np = h.in(b_np), o_outl = h.in(b_outl), o_dec = h.in(b_dec), o_ref = h.in(b_ref),
               o_kf = h.in(b_kf), o_pbad = h.in(b_pbad), o_pobs = h.in(b_pobs), o_base = h.in(b_base), o_slots = h.in(n_keys_total * 4);
  // the output group: what is short first; assigned is read too, so the whole block is uploaded
  const size_t o_head = h.out((size_t)S * sizeof(orbfe_kf_header)), o_nnew = h.out(create ? (size_t)S * 4 : 0),
               o_idx = h.out(create ? news * 4 : 0), o_asg = h.out(C.assigned ? rows * 4 : 0),
               o_sel = h.out((create && C.depth_selected) ? rows * 4 : 0), o_new = h.out(create ? news * sizeof(orbfe_map_point) : 0);
  if ((rc = h.open())) return rc;
  uint8_t *const hp = h.host(0), *const d = h.dev(0);
  auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(hp + off, src, bytes); };
  put(o_keys, C.keys_un, b_keys); put(o_desc, C.desc, b_desc); put(o_depth, C.depth, b_depth); put(o_n, C.n, b_n); put(o_cam, C.cam, b_cam);
  put(o_points, C.points, b_points); put(o_np, C.n_points, b_np); put(o_outl, C.outlier, b_outl); put(o_dec, C.decision, b_dec);
  put(o_pbad, C.point_bad, b_pbad); put(o_pobs, C.point_observations, b_pobs); put(o_base, C.n_points_base, b_base);
  put(o_asg, C.assigned, C.assigned ? rows * 4 : 0);
  if (decide) {
    put(o_ref, ref.data(), b_ref);
    orbfe_cov_keyframe* table = (orbfe_cov_keyframe*)(hp + o_kf);
    for (int k = 0; k < C.n_kf; k++) {   // only `slots` and `n_keys` are read: the other addresses are not staged and read as null
      const orbfe_cov_keyframe& K = C.keyframes[k];
      table[k] = K;
      table[k].keys_un = table[k].u_right = table[k].depth = 0;
      if (staged_at[k] >= 0) {
        memcpy(hp + o_slots + (size_t)staged_at[k] * 4, kf_slots_at(K.slots), (size_t)K.n_keys * 4);
        table[k].slots = (uint64_t)(uintptr_t)(d + o_slots + (size_t)staged_at[k] * 4);
      } else if (K.slots && !(K.slots & 3)) {
        table[k].slots = 0;   // a row no frame names, or one with nothing to walk: its host address means nothing on the device
      }
    }
  }
  if ((rc = h.upload(true))) return rc;
  KfLaunch L;
  memset(&L, 0, sizeof(L));
  L.C = C;
  L.cam = *camera;
  L.C.keys_un = (const orbfe_keypoint*)(d + o_keys); L.C.desc = d + o_desc; L.C.depth = (const float*)(d + o_depth);
  L.C.n = (const int32_t*)(d + o_n); L.C.cam = (const orbfe_unproject_cam*)(d + o_cam);
  L.C.assigned = C.assigned ? (int32_t*)(d + o_asg) : nullptr; L.C.points = d + o_points; L.C.n_points = (const int32_t*)(d + o_np);
  L.C.outlier = C.outlier ? d + o_outl : nullptr; L.C.decision = (const orbfe_kf_decision_in*)(d + o_dec);
  L.C.ref_kf = d + o_ref; L.C.ref_kf_stride = 4; L.C.keyframes = (const orbfe_cov_keyframe*)(d + o_kf); L.C.point_bad = d + o_pbad;
  L.C.point_observations = (const int32_t*)(d + o_pobs); L.C.n_points_base = b_base ? (const int32_t*)(d + o_base) : nullptr;
  L.C.headers = (orbfe_kf_header*)(d + o_head); L.C.new_points = (orbfe_map_point*)(d + o_new); L.C.new_index = (int32_t*)(d + o_idx);
  L.C.n_new = (int32_t*)(d + o_nnew); L.C.depth_selected = (create && C.depth_selected) ? (float*)(d + o_sel) : nullptr;
  const hipError_t lds = orbfe_launch_keyframe_insertion(L, h.stream);
  if (lds != hipSuccess) return hip_status("keyframe insertion: raising the kernel's dynamic LDS limit failed", lds);
  if ((rc = h.finish(h.out_bytes()))) return rc;
  const orbfe_kf_header* rh = (const orbfe_kf_header*)(hp + o_head);
  for (int f = 0; f < S; f++) {   // the header, and the heads that were written: what lies behind them stays the caller's
    C.headers[f] = rh[f];
    if (!create) continue;
    const int nn = ((const int32_t*)(hp + o_nnew))[f];
    C.n_new[f] = nn;
    if (rh[f].status == ORBFE_KF_REFUSED) continue;
    if (nn > 0) {
      memcpy(C.new_index + (size_t)f * C.new_cap, hp + o_idx + (size_t)f * C.new_cap * 4, (size_t)nn * 4);
      memcpy(C.new_points + (size_t)f * C.new_cap, hp + o_new + (size_t)f * C.new_cap * sizeof(orbfe_map_point), (size_t)nn * sizeof(orbfe_map_point));
    }
    if (C.depth_selected) memcpy(C.depth_selected + (size_t)f * C.cap, hp + o_sel + (size_t)f * C.cap * 4, (size_t)C.cap * 4);
    if (C.assigned && C.mode != ORBFE_KF_MODE_LAST_FRAME)
      memcpy(C.assigned + (size_t)f * C.cap, hp + o_asg + (size_t)f * C.cap * 4, (size_t)C.cap * 4);
  }
  return ORBFE_OK;
}
