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
//
// RunGlobalBundleAdjustmentUpdateMap is LoopClosing::RunGlobalBundleAdjustment's block LoopClosing.cc:648-703 and nothing around it:
// the caller keeps the stop / wait of local mapping, mMutexGBA, mpMap->mMutexMapUpdate, InformNewBigChange and Release.  It walks
// mvpKeyFrameOrigins / GetChilds() breadth-first as the reference does -- that fixes the set of keyframes reached and every parent's
// row --, marshals mnBAGlobalForKF == nLoopKF with mTcwGBA / mPosGBA into the row arrays and the two tables of orbfe_gba_update_map,
// and after that ONE call writes mTcwBefGBA, mTcwGBA (propagated keyframes), mnBAGlobalForKF and SetPose of every keyframe reached and
// SetWorldPos of every point that took its mPosGBA or moved with its reference keyframe, and of no other.  UpdateNormalAndDepth is not
// part of that block.  mHalfBaseline is protected in the reference; it is mb / 2 (KeyFrame.cc:52), read from the first origin.
// Deviations: a keyframe met a second time in the walk (a tree that is not a tree) is not listed again -- the reference would correct
// it twice, or walk a cycle for ever; a keyframe that is not optimised and hangs under no optimised one is left as it is, with the
// points it carries -- the reference reads an empty mTcwGBA there; a point whose reference keyframe the walk did not reach stays -- the
// reference reads that keyframe's mTcwBefGBA, stale or empty.  A failing library call is logged to stderr and leaves the map untouched.
// Members used:
//   Map:      mvpKeyFrameOrigins, GetAllMapPoints()
//   KeyFrame: GetChilds(), GetPose(), SetPose(cv::Mat), mb, mTcwGBA, mTcwBefGBA, mnBAGlobalForKF
//   MapPoint: isBad(), GetWorldPos(), SetWorldPos(cv::Mat), GetReferenceKeyFrame(), mPosGBA, mnBAGlobalForKF
#pragma once
#include <stdio.h>

#include <map>
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

// Returns the number of map points written, -1 when the library call failed.
template <class MapT>
int RunGlobalBundleAdjustmentUpdateMap(MapT* pMap, const unsigned long nLoopKF) {
  using KeyFrameT = std::remove_pointer_t<typename decltype(pMap->mvpKeyFrameOrigins)::value_type>;
  using MapPointT = std::remove_pointer_t<typename decltype(pMap->GetAllMapPoints())::value_type>;
  // Correct keyframes starting at map first keyframe (:648-670): the walk's order, every keyframe once
  std::vector<KeyFrameT*> vpKFs;
  std::vector<int32_t> parent;
  std::map<KeyFrameT*, int32_t> row;
  for (KeyFrameT* pKF : pMap->mvpKeyFrameOrigins) {
    if (!pKF || row.count(pKF)) continue;
    row[pKF] = (int32_t)vpKFs.size();
    vpKFs.push_back(pKF);
    parent.push_back(-1);
  }
  for (size_t i = 0; i < vpKFs.size(); i++) {
    const auto sChilds = vpKFs[i]->GetChilds();
    for (KeyFrameT* pChild : sChilds) {
      if (!pChild || row.count(pChild)) continue;
      row[pChild] = (int32_t)vpKFs.size();
      vpKFs.push_back(pChild);
      parent.push_back((int32_t)i);
    }
  }
  const int n_kf = (int)vpKFs.size();
  std::vector<float> poses((size_t)n_kf * 12), gba_poses;
  std::vector<int32_t> kf_gba_row(n_kf, -1);
  std::vector<cv::Mat> vTcwBef(n_kf);
  auto read_pose = [](const cv::Mat& T, float* o) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) o[4 * r + c] = T.template at<float>(r, c);
  };
  for (int k = 0; k < n_kf; k++) {
    vTcwBef[k] = vpKFs[k]->GetPose();
    read_pose(vTcwBef[k], &poses[(size_t)k * 12]);
    if (vpKFs[k]->mnBAGlobalForKF == nLoopKF) {
      kf_gba_row[k] = (int32_t)(gba_poses.size() / 12);
      gba_poses.resize(gba_poses.size() + 12);
      read_pose(vpKFs[k]->mTcwGBA, &gba_poses[gba_poses.size() - 12]);
    }
  }
  // Correct MapPoints (:672-703)
  const std::vector<MapPointT*> vpMPs = pMap->GetAllMapPoints();
  const int n_pt = (int)vpMPs.size();
  std::vector<float> points((size_t)n_pt * 3), gba_points;
  std::vector<int32_t> point_gba_row(n_pt, -1), ref(n_pt, -1);
  for (int i = 0; i < n_pt; i++) {
    MapPointT* pMP = vpMPs[i];
    if (!pMP || pMP->isBad()) continue;   // the position of a bad point is not read: it goes through as zeros and is not written
    const cv::Mat X = pMP->GetWorldPos();
    for (int r = 0; r < 3; r++) points[(size_t)i * 3 + r] = X.template at<float>(r);
    if (pMP->mnBAGlobalForKF == nLoopKF) {
      point_gba_row[i] = (int32_t)(gba_points.size() / 3);
      for (int r = 0; r < 3; r++) gba_points.push_back(pMP->mPosGBA.template at<float>(r));
    } else {
      const auto it = row.find(pMP->GetReferenceKeyFrame());
      if (it != row.end()) ref[i] = it->second;
    }
  }
  std::vector<orbfe_gba_map_keyframe> kf_out(n_kf);
  std::vector<float> points_out(points.size());
  orbfe_gba_map_result res;
  const float half_baseline = n_kf ? vpKFs[0]->mb / 2 : 0.f;
  const int rc = orbfe_gba_update_map(poses.data(), parent.data(), kf_gba_row.data(), n_kf, gba_poses.data(), (int)(gba_poses.size() / 12),
                                      half_baseline, points.data(), point_gba_row.data(), ref.data(), n_pt, gba_points.data(),
                                      (int)(gba_points.size() / 3), kf_out.data(), points_out.data(), &res);
  if (rc != ORBFE_OK) {
    fprintf(stderr, "orbfe RunGlobalBundleAdjustmentUpdateMap: %s (code %d)\n", orbfe_last_error(), rc);
    return -1;
  }
  for (int k = 0; k < n_kf; k++) {
    if (kf_out[k].status == ORBFE_GBA_MAP_KF_UNREACHED) continue;
    KeyFrameT* pKF = vpKFs[k];
    if (kf_out[k].status == ORBFE_GBA_MAP_KF_PROPAGATED) {
      cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) T.template at<float>(r, c) = kf_out[k].Tcw[4 * r + c];
      pKF->mTcwGBA = T;
      pKF->mnBAGlobalForKF = nLoopKF;
    }
    pKF->mTcwBefGBA = vTcwBef[k];
    pKF->SetPose(pKF->mTcwGBA);
  }
  int n_written = 0;
  for (int i = 0; i < n_pt; i++) {
    const bool taken = point_gba_row[i] >= 0;
    const bool moved = !taken && ref[i] >= 0 && kf_out[ref[i]].status != ORBFE_GBA_MAP_KF_UNREACHED;
    if (!taken && !moved) continue;
    cv::Mat X(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) X.template at<float>(r) = points_out[(size_t)i * 3 + r];
    vpMPs[i]->SetWorldPos(X);
    n_written++;
  }
  return n_written;
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
