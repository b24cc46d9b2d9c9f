// initial_map_internal.h -- the arithmetic of Tracking::CreateInitialMapMonocular around its bundle adjustment, once, for the kernels
// (initial_map_kernels.hip) and for host code that wants the same bits (tests/cpp_ba/host_arith.cpp).  __host__ __device__ inline
// functions compiled with -ffp-contract=off on both sides; no HIP call.  Every function handles ONE item: a match, a point.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   Tracking::MonocularInitialization      L/src/Tracking.cc:551-566   (matches that were not triangulated are dropped; the two poses)
//   Tracking::CreateInitialMapMonocular    L/src/Tracking.cc:584-612   (a point and two observations per match), :620-642 (the scale)
//   KeyFrame::ComputeSceneMedianDepth      L/src/KeyFrame.cc:588-615
//   KeyFrame::TrackedMapPoints             L/src/KeyFrame.cc:237-256
#pragma once
#include <string.h>

#include "lba_internal.h"

// ---- build
// A match that becomes a map point: an index into keys2, and triangulated
__host__ __device__ inline bool imap_is_point(int32_t match, int n2, uint64_t tri_word, int bit) {
  return match >= 0 && match < n2 && ((tri_word >> bit) & 1ull) != 0;
}
// mvInvLevelSigma2[octave], or NaN where the camera has no such level: the adjustment refuses a problem with such an edge
__host__ __device__ inline float imap_inv_sigma2(const orbfe_pose_camera& cam, int32_t octave) {
  return octave >= 0 && octave < cam.n_levels && octave < ORBFE_MAX_LEVELS ? cam.inv_level_sigma2[octave] : NAN;
}
// The two monocular observations of point p = match (i -> j): keyframe 0 sees it at keys1[i], keyframe 1 at keys2[j]
__host__ __device__ inline void imap_edges(const orbfe_pose_camera& cam, int p, const float* key1, int32_t octave1, const float* key2,
                                           int32_t octave2, orbfe_lba_edge* e) {
  e[0].kf = 0; e[0].point = p; e[0].u = key1[0]; e[0].v = key1[1]; e[0].u_right = -1.0f; e[0].inv_sigma2 = imap_inv_sigma2(cam, octave1);
  e[1].kf = 1; e[1].point = p; e[1].u = key2[0]; e[1].v = key2[1]; e[1].u_right = -1.0f; e[1].inv_sigma2 = imap_inv_sigma2(cam, octave2);
}
// The two keyframes: pose1 (NULL: the identity) and [R21 | t21]
__host__ __device__ inline void imap_poses(const float* pose1, const float* R21, const float* t21, float* poses) {
  for (int j = 0; j < 12; j++) poses[j] = pose1 ? pose1[j] : ((j == 0 || j == 5 || j == 10) ? 1.0f : 0.0f);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) poses[12 + 4 * r + c] = R21[3 * r + c];
    poses[12 + 4 * r + 3] = t21[r];
  }
}

// ---- finish
// KeyFrame.cc:604  float z = Rcw2.dot(x3Dw) + zcw: cv::Mat::dot accumulates in double in element order, the sum with the float zcw
// is a double, the assignment rounds once
__host__ __device__ inline float imap_depth(const float* Tcw, const float* X) {
  double s = 0.0;
  s += (double)Tcw[8] * (double)X[0];
  s += (double)Tcw[9] * (double)X[1];
  s += (double)Tcw[10] * (double)X[2];
  return (float)(s + (double)Tcw[11]);
}
// A float depth as an unsigned key of the same order (-0 before +0); NaN, on which std::sort is undefined, sorts last
__host__ __device__ inline uint32_t imap_depth_key(float z) {
  if (z != z) return 0xffffffffu;
  uint32_t b;
  memcpy(&b, &z, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float imap_key_depth(uint32_t k) {
  if (k == 0xffffffffu) return NAN;
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float z;
  memcpy(&z, &b, 4);
  return z;
}
// Tracking.cc:623: the reset rule.  n: points, tracked: pKFcur->TrackedMapPoints(1)
__host__ __device__ inline int imap_reason(int n, float median, int tracked, int min_points, int ba_rounds) {
  int reason = 0;
  if (n == 0) reason |= ORBFE_IMAP_NO_POINTS;
  if (median < 0) reason |= ORBFE_IMAP_MEDIAN_NEGATIVE;
  if (tracked < min_points) reason |= ORBFE_IMAP_FEW_POINTS;
  if (ba_rounds < 0) reason |= ORBFE_IMAP_REFUSED;
  return reason;
}
// :621, :631, :640: float invMedianDepth = 1.0f / medianDepth; a float product per coordinate
__host__ __device__ inline float imap_inv_median(float median) { return 1.0f / median; }
__host__ __device__ inline float imap_scaled(float x, float inv_median) { return x * inv_median; }

// ---- the launch (initial_map_kernels.hip)
struct ImapLaunch {
  const orbfe_pose_camera* camera;
  const float* keys1; const float* keys2;                          // [P][cap][2]
  const int32_t* n1; const int32_t* n2; int cap;                   // [P]
  const int32_t* matches12;                                        // [P][cap]
  const float* P3D; const uint64_t* triangulated;                  // [P][cap][3], [P][W]; W = ceil(cap / 64)
  const orbfe_init_result* init;                                   // [P]
  const int32_t* octaves1; const int32_t* octaves2;                // [P][cap]
  const float* pose1;                                              // [P][12] or null
  int n_iterations, q, min_points;
  float* poses; float* points; int32_t* index;                     // [P][2][12], [P][cap][3], [P][cap]
  float* poses_ba; float* points_ba;                               // the same, or null
  orbfe_initial_map_result* result;                                // [P]
  // workspace: the adjustment's problems and arrays, then its own workspace
  orbfe_lba_problem* problems;                                     // [P]
  float* ba_poses; uint8_t* ba_fixed; float* ba_points; orbfe_lba_edge* ba_edges;   // [P][2][12], [P][2], [P][cap][3], [P][2 cap]
  float* ba_poses_out; float* ba_points_out; orbfe_ba_result* ba_result;            // [P][2][12], [P][cap][3], [P]
  uint8_t* lba_workspace;
};
// the regions of the workspace behind `base`, and its size
__host__ inline size_t imap_ws_carve(uint8_t* base, int P, int cap, ImapLaunch* L) {
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return base ? base + o : nullptr; };
  uint8_t* r[9];
  r[0] = take((size_t)P * sizeof(orbfe_lba_problem));
  r[1] = take((size_t)P * 96);
  r[2] = take((size_t)P * 2);
  r[3] = take((size_t)P * cap * 12);
  r[4] = take((size_t)P * cap * 2 * sizeof(orbfe_lba_edge));
  r[5] = take((size_t)P * 96);
  r[6] = take((size_t)P * cap * 12);
  r[7] = take((size_t)P * sizeof(orbfe_ba_result));
  r[8] = take((size_t)P * lba_ws_bytes(2, cap, 2 * cap));
  if (L) {
    L->problems = (orbfe_lba_problem*)r[0]; L->ba_poses = (float*)r[1]; L->ba_fixed = r[2]; L->ba_points = (float*)r[3];
    L->ba_edges = (orbfe_lba_edge*)r[4]; L->ba_poses_out = (float*)r[5]; L->ba_points_out = (float*)r[6];
    L->ba_result = (orbfe_ba_result*)r[7]; L->lba_workspace = r[8];
  }
  return off;
}
void orbfe_launch_initial_map(const ImapLaunch& L, int P, hipStream_t s);
