// keyframe_internal.h -- the reading of the statistics tail of Tracking::TrackLocalMap, of Tracking::NeedNewKeyFrame and of the
// depth-ordered point creation of Tracking::CreateNewKeyFrame / UpdateLastFrame / StereoInitialization, once, for the kernel
// (keyframe_kernels.hip) and for host code that wants the same answers (tests/cpp_keyframe/host_arith.cpp).  __host__ __device__
// inline functions, compiled with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   Tracking::TrackLocalMap (statistics)   L/src/Tracking.cc:851-877
//   Tracking::NeedNewKeyFrame              L/src/Tracking.cc:880-962
//   Tracking::CreateNewKeyFrame (points)   L/src/Tracking.cc:973-1024
//   Tracking::UpdateLastFrame (points)     L/src/Tracking.cc:732-777
//   Tracking::StereoInitialization         L/src/Tracking.cc:455-479
//   KeyFrame::TrackedMapPoints             L/src/KeyFrame.cc:237-256
//   Frame::UnprojectStereo                 L/src/Frame.cc:668-679
//   MapPoint::MapPoint (from a frame)      L/src/MapPoint.cc:49-77
//
// The order of std::sort over pair<float, int> is, for depth > 0, the ascending order of (bits(depth) << 32) | index: positive IEEE
// floats order as their bit patterns, +inf (0x7f800000) behind every finite one, and the index breaks ties as pair's operator< does.
// The loop at :992-1022 / :751-777 counts nPoints in both branches, so behind entry j it is j + 1, and it breaks behind the first j
// with depth_j > th_depth && j + 1 > 100.  With c = |{depth <= th_depth}| the entries 0 .. c - 1 are those, entry j >= c has
// depth_j > th_depth, and the first j >= c with j >= 100 is max(100, c): the prefix is min(M, max(100, c) + 1) entries long.
#pragma once
#include "mappoint_internal.h"

#define KF_HD __host__ __device__ __forceinline__
#define KF_THREADS 1024                    // threads of the kernel's workgroup
#define KF_RECORD_DWORDS 18                // sizeof(orbfe_map_point) / 4
#define KF_KEY_PAD 0xffffffffffffffffull   // behind every key: no float has the bits 0xffffffff with depth > 0

KF_HD uint32_t kf_float_bits(float v) {
  union { float f; uint32_t u; } c;
  c.f = v;
  return c.u;
}
KF_HD float kf_bits_float(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = u;
  return c.f;
}
KF_HD bool kf_candidate(float depth) { return depth > 0; }   // :983, :738, :468 -- false for NaN
KF_HD uint64_t kf_key(float depth, int i) { return ((uint64_t)kf_float_bits(depth) << 32) | (uint32_t)i; }
KF_HD int kf_key_index(uint64_t key) { return (int)(uint32_t)key; }
KF_HD float kf_key_depth(uint64_t key) { return kf_bits_float((uint32_t)(key >> 32)); }
KF_HD bool kf_within(float depth, float th_depth) { return depth <= th_depth; }   // the negation of `first > mThDepth`, :1020
KF_HD int kf_prefix(int M, int c) { return M < (c > ORBFE_KF_CLOSE_POINTS ? c : ORBFE_KF_CLOSE_POINTS) + 1 ? M : (c > ORBFE_KF_CLOSE_POINTS ? c : ORBFE_KF_CLOSE_POINTS) + 1; }
KF_HD bool kf_close(float depth, float th_depth) { return depth > 0 && depth < th_depth; }   // :910
KF_HD bool kf_init_runs(int n) { return n > ORBFE_KF_INIT_MIN_KEYS; }   // :455

// the clamped counts of a frame and of the records its slots index
KF_HD int kf_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
KF_HD int kf_source_frame(int f, int frame_shift, int S) { return (int)(((long long)f - frame_shift % S + S) % S); }

// Observations() > 0 of the point in an occupied slot
KF_HD bool kf_observed(const uint8_t* records, int point_stride, int observed_offset, int32_t a) {
  if (observed_offset < 0) return true;
  return *reinterpret_cast<const int32_t*>(records + (size_t)a * point_stride + observed_offset) > 0;
}

// :854-866, one slot: does it count in mnMatchesInliers
KF_HD bool kf_inlier(bool occupied, bool outlier, bool observed, bool only_tracking) {
  return occupied && !outlier && (only_tracking || observed);
}
// :1000 / :759 on one entry of the prefix: is a point created there
KF_HD bool kf_creates(bool occupied, bool observed) { return !occupied || !observed; }

// Frame::UnprojectStereo in the arithmetic of unproject_stereo_kernel (frustum_kernels.hip)
KF_HD void kf_unproject(const orbfe_unproject_cam& c, float kx, float ky, float z, float* pos) {
  const float x = (kx - c.cx) * z * c.invfx;
  const float y = (ky - c.cy) * z * c.invfy;
#pragma unroll
  for (int r = 0; r < 3; r++) {   // mRwc * x3Dc + mOw: cv::gemm small-matrix path (float dot, double epilogue)
    const float t = c.Rwc[3 * r] * x + c.Rwc[3 * r + 1] * y + c.Rwc[3 * r + 2] * z;
    pos[r] = (float)((double)t * 1.0 + (double)c.Ow[r] * 1.0);
  }
}

// the floats of a new point.  Keyframe form: UpdateNormalAndDepth over one observation (mappoint_internal.h); frame form: the
// constructor at MapPoint.cc:58-69, the same expressions without `0.0f +` and `* (float)(1.0 / 1)`
KF_HD void kf_point_floats(const orbfe_unproject_cam& c, float kx, float ky, float z, float sf_octave, float sf_top, bool frame_form, float* out8) {
  kf_unproject(c, kx, ky, z, out8);
  float t[3];
  mp_unit_term(out8, c.Ow, t);
  if (frame_form) {
    out8[3] = t[0]; out8[4] = t[1]; out8[5] = t[2];
  } else {
    const float inv_n = mp_inv_count(1);
    out8[3] = (0.0f + t[0]) * inv_n; out8[4] = (0.0f + t[1]) * inv_n; out8[5] = (0.0f + t[2]) * inv_n;
  }
  mp_depth_range(out8, c.Ow, sf_octave, sf_top, &out8[6], &out8[7]);
}

// :870-877
KF_HD bool kf_recent_reloc(const orbfe_kf_decision_in& D) {
  return D.frame_id < (uint64_t)(uint32_t)(D.last_reloc_frame_id + (uint32_t)D.max_frames);   // long unsigned < unsigned + int
}
KF_HD int kf_track_ok(const orbfe_kf_decision_in& D, int n_matches_inliers) {
  if (kf_recent_reloc(D) && n_matches_inliers < 50) return 0;
  return n_matches_inliers < 30 ? 0 : 1;
}
KF_HD int kf_min_obs(int n_kfs) { return n_kfs <= 2 ? 2 : 3; }   // :896-898

// :881-961 behind the counts.  H: n_matches_inliers, n_tracked_close, n_non_tracked_close and n_ref_matches are read; early,
// conditions, need and interrupt_ba are written
KF_HD void kf_decide(const orbfe_kf_decision_in& D, orbfe_kf_header& H) {
  H.early = ORBFE_KF_EARLY_NONE; H.conditions = 0; H.need = 0; H.interrupt_ba = 0;
  if (D.only_tracking) { H.early = ORBFE_KF_EARLY_ONLY_TRACKING; return; }
  if (D.mapper_stopped) { H.early = ORBFE_KF_EARLY_STOPPED; return; }
  const int nKFs = D.n_kfs;
  if (kf_recent_reloc(D) && nKFs > D.max_frames) { H.early = ORBFE_KF_EARLY_RELOCALISED; return; }
  const int nRefMatches = H.n_ref_matches, mnMatchesInliers = H.n_matches_inliers;
  const bool bLocalMappingIdle = D.accept_keyframes != 0;
  const bool mono = D.sensor == ORBFE_KF_SENSOR_MONOCULAR;
  const bool bNeedToInsertClose = (H.n_tracked_close < 100) && (H.n_non_tracked_close > 70);
  float thRefRatio = 0.75f;
  if (nKFs < 2) thRefRatio = 0.4f;
  if (mono) thRefRatio = 0.9f;
  const bool c1a = D.frame_id >= (uint64_t)(uint32_t)(D.last_keyframe_id + (uint32_t)D.max_frames);
  const bool c1b = D.frame_id >= (uint64_t)(uint32_t)(D.last_keyframe_id + (uint32_t)D.min_frames) && bLocalMappingIdle;
  const bool c1c = !mono && ((double)mnMatchesInliers < (double)nRefMatches * 0.25 || bNeedToInsertClose);
  const bool c2 = (((float)mnMatchesInliers < (float)nRefMatches * thRefRatio || bNeedToInsertClose) && mnMatchesInliers > 15);
  H.conditions = (c1a ? ORBFE_KF_C1A : 0) | (c1b ? ORBFE_KF_C1B : 0) | (c1c ? ORBFE_KF_C1C : 0) | (c2 ? ORBFE_KF_C2 : 0);
  if ((c1a || c1b || c1c) && c2) {
    if (bLocalMappingIdle) { H.need = 1; return; }
    H.interrupt_ba = 1;
    H.need = (!mono && D.keyframes_in_queue < 3) ? 1 : 0;
  }
}

KF_HD void kf_header_clear(orbfe_kf_header& H, int status) {
  H.n_matches_inliers = H.track_ok = H.n_tracked_close = H.n_non_tracked_close = H.n_ref_matches = H.early = H.conditions = H.need = 0;
  H.interrupt_ba = H.M = H.c = H.L = H.n_created = H.n_cleared = H.reserved = 0;
  H.status = status;
}

KF_HD const int32_t* kf_slots_at(uint64_t address) { return reinterpret_cast<const int32_t*>((uintptr_t)address); }
// a reference row may be walked
KF_HD bool kf_ref_row_ok(const orbfe_cov_keyframe& K) { return K.n_keys == 0 || (K.n_keys > 0 && K.slots && !(K.slots & 3)); }
KF_HD bool kf_ref_slot_ok(int32_t p, int n_map_points) { return p >= -1 && p < n_map_points; }
KF_HD bool kf_ref_counts(int32_t p, const uint8_t* point_bad, const int32_t* point_observations, int min_obs) {
  return p >= 0 && !point_bad[p] && point_observations[p] >= min_obs;
}

// ---- the launch: the call's arrays (device addresses) and the camera, by value
struct KfLaunch {
  orbfe_kf_call C;
  orbfe_kf_scales cam;
};

// The whole reading for frame f, sequentially: what the kernel spreads over a workgroup.  keys: room for the frame's candidates
// (cap entries); mark: (cap + 31) / 32 words.  Every address of L.C is one this code may read (host memory for host callers).
inline void kf_frame_sequential(const KfLaunch& L, int f, uint64_t* keys, uint32_t* mark) {
  const orbfe_kf_call& C = L.C;
  const int n = kf_clamp(C.n[f], C.cap), S = C.S;
  const int fs = kf_source_frame(f, C.frame_shift, S);
  const int n_pts = C.assigned ? kf_clamp(C.n_points[fs], C.p_cap) : 0;
  const uint8_t* records = (const uint8_t*)C.points + (size_t)fs * C.p_cap * C.point_stride;
  const size_t row = (size_t)f * C.cap;
  const bool stats = C.flags & ORBFE_KF_STATISTICS, decide = C.flags & ORBFE_KF_DECISION, create = C.flags & ORBFE_KF_CREATE;
  orbfe_kf_header H;
  kf_header_clear(H, ORBFE_KF_REFUSED);
  C.headers[f] = H;
  if (create) C.n_new[f] = 0;
  auto slot = [&](int i) { return C.assigned ? C.assigned[row + i] : -1; };
  auto is_outlier = [&](int i) { return C.outlier && C.outlier[row + i]; };
  for (int i = 0; i < n; i++)
    if (slot(i) >= n_pts) return;
  const orbfe_cov_keyframe* K = nullptr;
  if (decide) {
    const int32_t r = *reinterpret_cast<const int32_t*>((const uint8_t*)C.ref_kf + (size_t)f * C.ref_kf_stride);
    if (r < -1 || r >= C.n_kf) return;
    if (r >= 0) {
      K = C.keyframes + r;
      if (!kf_ref_row_ok(*K)) return;
      for (int i = 0; i < K->n_keys; i++)
        if (!kf_ref_slot_ok(kf_slots_at(K->slots)[i], C.n_map_points)) return;
    }
  }
  kf_header_clear(H, ORBFE_KF_OK);
  if (stats) {
    const orbfe_kf_decision_in& D = C.decision[f];
    for (int i = 0; i < n; i++) {
      const int32_t a = slot(i);
      if (kf_inlier(a >= 0, is_outlier(i), a >= 0 && kf_observed(records, C.point_stride, C.observed_offset, a), D.only_tracking != 0))
        H.n_matches_inliers++;
    }
    H.track_ok = kf_track_ok(D, H.n_matches_inliers);
    if (decide) {
      if (D.sensor != ORBFE_KF_SENSOR_MONOCULAR)
        for (int i = 0; i < n; i++)
          if (kf_close(C.depth[row + i], L.cam.th_depth)) {
            if (slot(i) >= 0 && !is_outlier(i)) H.n_tracked_close++; else H.n_non_tracked_close++;
          }
      if (K)
        for (int i = 0; i < K->n_keys; i++)
          H.n_ref_matches += kf_ref_counts(kf_slots_at(K->slots)[i], C.point_bad, C.point_observations, kf_min_obs(D.n_kfs)) ? 1 : 0;
      kf_decide(D, H);
    }
  }
  const bool init = C.mode == ORBFE_KF_MODE_STEREO_INIT;
  const bool run = create && (!decide || H.need) && (!init || kf_init_runs(n));
  if (create && C.depth_selected)
    for (int i = 0; i < C.cap; i++) mark[i >> 5] = 0u;
  if (run) {
    int M = 0, c = 0;
    for (int i = 0; i < n; i++) {
      const float z = C.depth[row + i];
      if (!kf_candidate(z)) continue;
      keys[M++] = kf_key(z, i);
      c += kf_within(z, L.cam.th_depth) ? 1 : 0;
    }
    if (!init)   // insertion sort: the keys are distinct, so every correct sort gives this order
      for (int j = 1; j < M; j++) {
        const uint64_t k = keys[j];
        int at = j;
        while (at > 0 && keys[at - 1] > k) { keys[at] = keys[at - 1]; at--; }
        keys[at] = k;
      }
    const int Lp = init ? M : kf_prefix(M, c);
    int n_created = 0, n_cleared = 0;
    for (int j = 0; j < Lp; j++) {   // nothing is written before every created entry's octave is known to be in range
      const int i = kf_key_index(keys[j]);
      const int32_t a = init ? -1 : slot(i);
      const bool occupied = a >= 0, observed = occupied && kf_observed(records, C.point_stride, C.observed_offset, a);
      if (!kf_creates(occupied, observed)) continue;
      const int32_t octave = C.keys_un[row + i].octave;
      if (octave < 0 || octave >= L.cam.n_levels) {
        kf_header_clear(H, ORBFE_KF_REFUSED);
        C.headers[f] = H;
        return;
      }
    }
    const int32_t base = C.n_points_base ? C.n_points_base[f] : 0;
    for (int j = 0; j < Lp; j++) {
      const int i = kf_key_index(keys[j]);
      if (C.depth_selected) mark[i >> 5] |= 1u << (i & 31);
      const int32_t a = init ? -1 : slot(i);
      const bool occupied = a >= 0, observed = occupied && kf_observed(records, C.point_stride, C.observed_offset, a);
      if (!kf_creates(occupied, observed)) continue;
      const bool writes_slot = C.assigned && C.mode != ORBFE_KF_MODE_LAST_FRAME;
      if (occupied && C.mode == ORBFE_KF_MODE_KEYFRAME) {
        n_cleared++;
        C.assigned[row + i] = -1;
      }
      if (n_created < C.new_cap) {
        const orbfe_keypoint& kp = C.keys_un[row + i];
        orbfe_map_point& P = C.new_points[(size_t)f * C.new_cap + n_created];
        float v[8];
        kf_point_floats(C.cam[f], kp.x, kp.y, C.depth[row + i], L.cam.scale_factors[kp.octave], L.cam.scale_factors[L.cam.n_levels - 1],
                        C.mode == ORBFE_KF_MODE_LAST_FRAME, v);
        P.pos[0] = v[0]; P.pos[1] = v[1]; P.pos[2] = v[2]; P.normal[0] = v[3]; P.normal[1] = v[4]; P.normal[2] = v[5];
        P.min_distance = v[6]; P.max_distance = v[7];
        P.skip = 0;
        P.observed = C.mode == ORBFE_KF_MODE_LAST_FRAME ? 0 : 1;
        for (int b = 0; b < 32; b++) P.desc[b] = C.desc[(row + i) * 32 + b];
        C.new_index[(size_t)f * C.new_cap + n_created] = i;
        if (writes_slot) C.assigned[row + i] = base + n_created;
      }
      n_created++;
    }
    H.M = M; H.c = c; H.L = Lp; H.n_created = n_created; H.n_cleared = n_cleared;
    C.n_new[f] = n_created < C.new_cap ? n_created : C.new_cap;
    if (n_created > C.new_cap) H.status = ORBFE_KF_OVERFLOW;
  }
  if (create && C.depth_selected)
    for (int i = 0; i < C.cap; i++) C.depth_selected[row + i] = (run && ((mark[i >> 5] >> (i & 31)) & 1u)) ? C.depth[row + i] : -1.0f;
  C.headers[f] = H;
}

// not hipSuccess: the dynamic LDS limit of the kernel could not be raised on the current device, and nothing was launched
hipError_t orbfe_launch_keyframe_insertion(const KfLaunch& L, hipStream_t s);
