// Optimizer_hip.h -- host-side adapter that puts ORB_SLAM2::Optimizer::PoseOptimization on liborbfe.
//
// The reference's function (Source/Libraries/ORB_SLAM2/src/Optimizer.cc:233-435) builds a g2o graph of one pose vertex and one
// unary edge per keypoint with a map point, optimises it and writes the pose and the outlier flags back into the Frame.  This
// template marshals the members that function reads into the POD arguments of orbfe_pose_optimization (include/orbfe.h), runs the
// optimisation on the GPU and writes the result exactly where the reference writes it.  A template over the Frame type so that it
// compiles (and is unit-tested, tests/cpp_pose) without the reference tree; INTEGRATION.md shows the body a maintainer replaces.
//
// Members used (same names as the reference):
//   Frame:    N, mvKeysUn, mvuRight, mvpMapPoints, mvbOutlier, mvInvLevelSigma2, fx, fy, cx, cy, mbf, mTcw, SetPose(cv::Mat)
//   MapPoint: GetWorldPos(), the static mutex mGlobalMutex (held while the positions are read, as Optimizer.cc:273 does)
#pragma once
#include <stdio.h>

#include <mutex>
#include <type_traits>
#include <vector>

#include "../../../include/orbfe.h"

namespace ORB_SLAM2 {
namespace orbfe_host {

// int Optimizer::PoseOptimization(Frame* pFrame).  Errors (no device, a frame beyond the library's limits) are logged and return 0
// with the Frame untouched, like a frame with fewer than 3 correspondences.
template <class FrameT>
int PoseOptimization(FrameT* pFrame) {
  static_assert(sizeof(pFrame->mvKeysUn[0]) == sizeof(orbfe_keypoint), "cv::KeyPoint layout");
  using MapPointT = std::remove_pointer_t<typename std::remove_reference_t<decltype(pFrame->mvpMapPoints)>::value_type>;
  const int N = pFrame->N;
  std::vector<int32_t> assigned((size_t)N, -1);
  std::vector<float> pos;   // one position per keypoint with a map point, in keypoint order
  pos.reserve(3 * (size_t)N);
  {
    std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);
    for (int i = 0; i < N; i++) {
      MapPointT* pMP = pFrame->mvpMapPoints[i];
      if (!pMP) continue;
      const cv::Mat Xw = pMP->GetWorldPos();
      assigned[i] = (int32_t)(pos.size() / 3);
      pos.push_back(Xw.template at<float>(0));
      pos.push_back(Xw.template at<float>(1));
      pos.push_back(Xw.template at<float>(2));
    }
  }
  orbfe_pose_camera cam;
  cam.fx = pFrame->fx;
  cam.fy = pFrame->fy;
  cam.cx = pFrame->cx;
  cam.cy = pFrame->cy;
  cam.mbf = pFrame->mbf;
  cam.n_levels = (int32_t)pFrame->mvInvLevelSigma2.size();
  for (int l = 0; l < ORBFE_MAX_LEVELS; l++) cam.inv_level_sigma2[l] = l < cam.n_levels ? pFrame->mvInvLevelSigma2[l] : 0.0f;
  float Tcw[12];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) Tcw[4 * r + c] = pFrame->mTcw.template at<float>(r, c);
  orbfe_frame_view v;
  v.n = N;
  v.keys_un = reinterpret_cast<const orbfe_keypoint*>(pFrame->mvKeysUn.data());
  v.desc = nullptr;
  v.u_right = pFrame->mvuRight.empty() ? nullptr : pFrame->mvuRight.data();
  v.min_x = v.max_x = v.min_y = v.max_y = 0.0f;
  orbfe_pose_result res;
  std::vector<uint8_t> outlier((size_t)N, 0);
  const int rc = orbfe_pose_optimization(&v, assigned.data(), pos.data(), 12, (int)(pos.size() / 3), &cam, Tcw, &res, outlier.data());
  if (rc != ORBFE_OK) {
    fprintf(stderr, "orbfe PoseOptimization: %s (code %d)\n", orbfe_last_error(), rc);
    return 0;
  }
  for (int i = 0; i < N; i++)
    if (assigned[i] >= 0) pFrame->mvbOutlier[i] = outlier[i] != 0;   // entries without a point stay as they are (Optimizer.cc:277)
  if (res.n_initial < 3) return 0;                                    // :357, before SetPose
  cv::Mat pose = cv::Mat::eye(4, 4, CV_32F);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) pose.template at<float>(r, c) = res.Tcw[4 * r + c];
  pFrame->SetPose(pose);
  return res.n_inliers;
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
