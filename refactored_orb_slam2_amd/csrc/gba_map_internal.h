// gba_map_internal.h -- the arithmetic of the map update behind the global bundle adjustment, once, for the kernels
// (gba_map_kernels.hip), for the host side (gba_map.cpp: the launch interface) and for host code that wants the same bits
// (tests/cpp_gba_map/host_arith.cpp).  __host__ __device__ inline functions, compiled with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   LoopClosing::RunGlobalBundleAdjustment, the block that applies the adjustment   L/src/LoopClosing.cc:648-703
//   KeyFrame::SetPose                                                               L/src/KeyFrame.cc:75-88
// cv::Mat arithmetic is read as mapping_internal.h and sim3_internal.h read it: a matrix product is a float dot product per element in
// index order, the epilogue alpha * dot + beta * addend is done in double and rounded once -- for alpha = -1 that is the exact
// negation, for one float addend it is the float sum (a double holds the sum of two floats closely enough that the second rounding
// changes nothing).  R * x + t is therefore sim3_transform_point and (R^T * x)[r] is tri_rt_row; neither is restated here.
// A pose is 12 floats, the rows of [R | t]; the fourth row of a 4 x 4 operand is 0 0 0 1 and takes part in every dot like any other
// term: a * 0 is added, not dropped (it turns a sum of -0 into +0 and keeps a NaN), a * 1 is a.  The fourth row of a product is not
// kept: with finite operands it is 0 0 0 1 again, and the next product takes it as that.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/orbfe.h"
#include "mapping_internal.h"
#include "sim3_internal.h"

#define GM_HD __host__ __device__ __forceinline__
#define GM_PENDING 3            // between the prepare and the finish kernel: Tcw holds Tchildc; never leaves the library
#define GM_CHAIN_THREADS 1024   // the one workgroup of the chain: 64 keyframes a lane at ORBFE_GBA_MAP_MAX_KEYFRAMES, a 64-bit mask
static_assert(ORBFE_GBA_MAP_MAX_KEYFRAMES <= 64 * GM_CHAIN_THREADS, "a lane of the chain keeps its keyframes in one 64-bit mask");

// the rotation and translation of a pose as the 3 x 3 and 3 x 1 operands of a gemm
GM_HD void gm_split(const float* T, float* R, float* t) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    R[3 * r] = T[4 * r];
    R[3 * r + 1] = T[4 * r + 1];
    R[3 * r + 2] = T[4 * r + 2];
    t[r] = T[4 * r + 3];
  }
}

// KeyFrame::SetPose (:75-88): Rwc = Rcw.t(), Ow = -Rwc * tcw, Twc = [Rwc Ow; 0 0 0 1], Cw = Twc * (half_baseline, 0, 0, 1)^T
GM_HD void gm_set_pose(const float* Tcw, float half_baseline, float* Twc, float* Cw) {
  float R[9], t[3];
  gm_split(Tcw, R, t);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    Twc[4 * r] = R[r];
    Twc[4 * r + 1] = R[3 + r];
    Twc[4 * r + 2] = R[6 + r];
    Twc[4 * r + 3] = (float)((double)tri_rt_row(R, r, t[0], t[1], t[2]) * -1.0);
  }
#pragma unroll
  for (int r = 0; r < 3; r++) Cw[r] = Twc[4 * r] * half_baseline + Twc[4 * r + 1] * 0.f + Twc[4 * r + 2] * 0.f + Twc[4 * r + 3] * 1.f;
}

// C = A * B, 4 x 4 float operands whose fourth rows are 0 0 0 1; C may be neither A nor B
GM_HD void gm_mul(const float* A, const float* B, float* C) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 4; c++)
      C[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c] + A[4 * r + 3] * (c == 3 ? 1.f : 0.f);
  }
}

// Tchildc = pChild->GetPose() * pKF->GetPoseInverse() (:655, :660): both poses from before the walk; Twc is SetPose's of the old pose
GM_HD void gm_relative(const float* child_Tcw, const float* parent_Tcw, float half_baseline, float* Tchildc) {
  float Twc[12], Cw[3];
  gm_set_pose(parent_Tcw, half_baseline, Twc, Cw);
  gm_mul(child_Tcw, Twc, Tchildc);
}

// pChild->mTcwGBA = Tchildc * pKF->mTcwGBA (:661): one link of the chain
GM_HD void gm_propagate(const float* Tchildc, const float* parent_TcwGBA, float* child_TcwGBA) { gm_mul(Tchildc, parent_TcwGBA, child_TcwGBA); }

// Xc = Rcw_bef * Xw + tcw_bef, Xw' = Rwc_new * Xc + twc_new (:692-701)
GM_HD void gm_move_point(const float* Tcw_bef, const float* Twc_new, const float* Xw, float* out) {
  float R[9], t[3], Xc[3];
  gm_split(Tcw_bef, R, t);
  sim3_transform_point(R, t, Xw, Xc);
  gm_split(Twc_new, R, t);
  sim3_transform_point(R, t, Xc, out);
}

// ---- the launch interface (gba_map_kernels.hip), device pointers
struct GmLaunch {
  int n_kf, n_gba_kf, n_points, point_stride, n_gba_points;
  float half_baseline;
  const float* poses;
  const int32_t* parent;
  const int32_t* kf_gba_row;
  const float* gba_poses;
  const uint8_t* points;
  const int32_t* point_gba_row;
  const int32_t* ref;
  const float* gba_points;
  orbfe_gba_map_keyframe* kf_out;
  float* points_out;
  orbfe_gba_map_result* result;
};
void orbfe_launch_gba_map(const GmLaunch& L, hipStream_t s);   // at most four launches; asynchronous
