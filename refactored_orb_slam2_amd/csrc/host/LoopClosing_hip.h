// LoopClosing_hip.h -- host-side adapter: the pose and map-point propagation of LoopClosing::CorrectLoop on liborbfe.
//
// The reference (Source/Libraries/ORB_SLAM2/src/LoopClosing.cc:417-491) walks the current keyframe and its covisible neighbours, gives
// each its corrected and its non-corrected Sim3, moves every map point they see through correctedSwi.map(Siw.map(P)) one point at a
// time on the host, marks it (mnCorrectedByKF, mnCorrectedReference), refreshes its normal and depth and sets the keyframe's pose.
// CorrectLoopPropagate is that block without the UpdateConnections calls (Covisibility_hip.h has their batch form): the two pose maps
// are built by the caller's own Sim3 type, as the reference builds them; all points move in ONE call of orbfe_sim3_correct_points --
// the expression of Optimizer::OptimizeEssentialGraph's map correction --; their UpdateNormalAndDepth is ONE batch (MapPoint_hip.h).
// The caller holds mpMap->mMutexMapUpdate, as LoopClosing.cc:415 does.
// Deviation: the reference refreshes the points of a keyframe behind the SetPose of the keyframes BEFORE it in the map and ahead of
// the SetPose of those after it, so the camera centres that enter a normal are a mix of old and new poses that depends on pointer
// order.  Here every SetPose comes first and the one batch refresh sees the corrected pose of every keyframe of the set, as
// OptimizeEssentialGraphApply does.  mnCorrectedByKF / mnCorrectedReference are written only after the library call has succeeded.
//
// A template over the KeyFrame and the pose map so that it compiles (and is unit-tested, tests/cpp/test_egraph_dropin.cpp) without the
// reference tree.  A failing library call is logged to stderr, never thrown; the two pose maps are then filled and nothing else is
// touched.
//
// Members used (same names as the reference):
//   KeyFrame: mnId, GetPose(), GetPoseInverse(), GetMapPointMatches(), SetPose(cv::Mat)
//   MapPoint: isBad(), GetWorldPos(), SetWorldPos(cv::Mat), mnCorrectedByKF, mnCorrectedReference, and what MapPoint_hip.h names
//   Sim3:     what Optimizer_hip.h's OptimizeEssentialGraph names, operator*, and rotation().toRotationMatrix()
#pragma once
#include <stdio.h>

#include <vector>

#include "Optimizer_hip.h"

namespace ORB_SLAM2 {
namespace orbfe_host {

// Returns the number of map points moved, -1 when the library call failed.
template <class KeyFrameT, class PoseMapT>
int CorrectLoopPropagate(KeyFrameT* pCurrentKF, const std::vector<KeyFrameT*>& vpCurrentConnectedKFs,
                         const typename PoseMapT::mapped_type& g2oScw, PoseMapT& CorrectedSim3, PoseMapT& NonCorrectedSim3) {
  typedef typename PoseMapT::mapped_type Sim3T;
  using MapPointT = std::remove_pointer_t<typename decltype(pCurrentKF->GetMapPointMatches())::value_type>;
  CorrectedSim3[pCurrentKF] = g2oScw;
  const cv::Mat Twc = pCurrentKF->GetPoseInverse();
  for (KeyFrameT* pKFi : vpCurrentConnectedKFs) {   // :417-441
    const cv::Mat Tiw = pKFi->GetPose();
    if (pKFi != pCurrentKF) {
      cv::Mat Ric(3, 3, CV_32F), tic(3, 1, CV_32F);   // Tic = Tiw * Twc: cv::Mat's float product, a dot product in index order
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 4; c++) {
          float a = 0.f;
          for (int k = 0; k < 4; k++) a += Tiw.template at<float>(r, k) * Twc.template at<float>(k, c);
          if (c < 3)
            Ric.template at<float>(r, c) = a;
          else
            tic.template at<float>(r) = a;
        }
      }
      CorrectedSim3[pKFi] = EssentialGraphSim3<Sim3T>(Ric, tic) * g2oScw;
    }
    cv::Mat Riw(3, 3, CV_32F), tiw(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) Riw.template at<float>(r, c) = Tiw.template at<float>(r, c);
      tiw.template at<float>(r) = Tiw.template at<float>(r, 3);
    }
    NonCorrectedSim3[pKFi] = EssentialGraphSim3<Sim3T>(Riw, tiw);
  }
  // the tables and the points, in the order of the reference's loop (:445-475): a point belongs to the first keyframe that reaches it
  std::vector<KeyFrameT*> vpKFs;
  std::vector<orbfe_eg_sim3> from, to;
  std::vector<MapPointT*> vpMPs;
  std::vector<float> points;
  std::vector<int32_t> ref;
  std::set<MapPointT*> seen;   // the marks are written once the library call has succeeded
  for (auto mit = CorrectedSim3.begin(), mend = CorrectedSim3.end(); mit != mend; mit++) {
    KeyFrameT* pKFi = mit->first;
    vpKFs.push_back(pKFi);
    to.push_back(EssentialGraphRecord(mit->second));
    from.push_back(EssentialGraphRecord(NonCorrectedSim3[pKFi]));
    const std::vector<MapPointT*> vpMPsi = pKFi->GetMapPointMatches();
    for (MapPointT* pMPi : vpMPsi) {
      if (!pMPi || pMPi->isBad() || pMPi->mnCorrectedByKF == pCurrentKF->mnId || seen.count(pMPi)) continue;
      const cv::Mat P3Dw = pMPi->GetWorldPos();
      for (int r = 0; r < 3; r++) points.push_back(P3Dw.template at<float>(r));
      ref.push_back((int32_t)vpKFs.size() - 1);
      vpMPs.push_back(pMPi);
      seen.insert(pMPi);
    }
  }
  std::vector<float> moved(points.size());
  const int rc = orbfe_sim3_correct_points(points.data(), (int)vpMPs.size(), ref.data(), from.data(), to.data(), (int)from.size(), moved.data());
  if (rc != ORBFE_OK) {
    fprintf(stderr, "orbfe CorrectLoopPropagate: %s (code %d)\n", orbfe_last_error(), rc);
    return -1;
  }
  // Update keyframe pose with corrected Sim3: [R t/s; 0 1] (:477-487)
  size_t k = 0;
  for (auto mit = CorrectedSim3.begin(), mend = CorrectedSim3.end(); mit != mend; mit++, k++) {
    const auto R = mit->second.rotation().toRotationMatrix();
    const double inv_s = 1. / mit->second.scale();
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T.template at<float>(r, c) = (float)R(r, c);
      T.template at<float>(r, 3) = (float)(mit->second.translation()[r] * inv_s);
    }
    vpKFs[k]->SetPose(T);
  }
  for (size_t i = 0; i < vpMPs.size(); i++) {
    cv::Mat X(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) X.template at<float>(r) = moved[3 * i + r];
    vpMPs[i]->SetWorldPos(X);
    vpMPs[i]->mnCorrectedByKF = pCurrentKF->mnId;
    vpMPs[i]->mnCorrectedReference = vpKFs[ref[i]]->mnId;
  }
  UpdateNormalAndDepth(vpMPs);   // behind every SetPose: see the header
  return (int)vpMPs.size();
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
