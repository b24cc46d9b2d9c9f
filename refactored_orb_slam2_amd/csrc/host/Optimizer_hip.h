// Optimizer_hip.h -- host-side adapters that put ORB_SLAM2::Optimizer::PoseOptimization, Optimizer::OptimizeSim3 and
// Optimizer::LocalBundleAdjustment on liborbfe.
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
//
// OptimizeSim3 (Optimizer.cc:1381-1573) is the same kind of adapter for orbfe_optimize_sim3; it is a template over the KeyFrame, the
// MapPoint and the g2o::Sim3 type and is unit-tested by tests/cpp_optsim3.  Members used:
//   KeyFrame: mK, GetRotation(), GetTranslation(), GetMapPointMatches(), mvKeysUn, mvInvLevelSigma2
//   MapPoint: isBad(), GetWorldPos(), GetIndexInKeyFrame(pKF)
//   Sim3:     rotation() (with toRotationMatrix()), translation(), scale(), and the constructor (Matrix3, Vector3, double)
//
// LocalBundleAdjustment (Optimizer.cc:437-760) is the adapter for orbfe_local_bundle_adjustment; a template over the KeyFrame and the
// Map type (the MapPoint type is the one the KeyFrame's matches point to), unit-tested by tests/cpp_lba.  Members used:
//   KeyFrame: mnId, mnBALocalForKF, mnBAFixedForKF, isBad(), GetVectorCovisibleKeyFrames(), GetMapPointMatches(), GetPose(),
//             SetPose(cv::Mat), mvKeysUn, mvuRight, mvInvLevelSigma2, fx, fy, cx, cy, mbf, EraseMapPointMatch(MapPoint*)
//   MapPoint: mnBALocalForKF, isBad(), GetObservations(), GetWorldPos(), SetWorldPos(cv::Mat), UpdateNormalAndDepth(),
//             EraseObservation(KeyFrame*)
//   Map:      mMutexMapUpdate
#pragma once
#include <stdio.h>
#include <string.h>

#include <list>
#include <map>
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

// int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
// const bool bFixScale).  The filters of :1436-1468 run here; the library gets the correspondences that pass them.  vpMatches1 and
// g2oS12 are written exactly where the reference writes them: the entries of the correspondences dropped in either classification
// are nulled, and with fewer than 10 left after the first one the function returns 0 WITHOUT writing g2oS12 (:1545).
// The ABI carries the similarity as floats.  LoopClosing::ComputeSim3 builds g2oS12 from the float matrices of the solver, so nothing
// is lost on the way in; on the way out the estimate is rounded to float and g2oS12 rebuilt by Sim3(R, t, s), whose quaternion is
// normalised -- 1e-7 relative, against the reference's unrounded doubles.
// Errors (no device, more correspondences than the library's limit) are logged and return 0 with nothing written.
// The graph construction of :1396-1514 as the library's arguments: the two views, the correspondences that pass the filters and,
// for each, its index in vpMatches1 (vnIndexEdge).
template <class KeyFrameT, class MapPointT>
void OptimizeSim3Marshal(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatches1, orbfe_sim3_view& v1,
                         orbfe_sim3_view& v2, std::vector<orbfe_optsim3_pair>& pairs, std::vector<size_t>& vnIndexEdge) {
  auto view = [](KeyFrameT* pKF) {
    orbfe_sim3_view v;
    memset(&v, 0, sizeof(v));
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation();
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) v.Rcw[3 * r + c] = R.template at<float>(r, c);
      v.tcw[r] = t.template at<float>(r);
    }
    v.fx = pKF->mK.template at<float>(0, 0); v.fy = pKF->mK.template at<float>(1, 1);
    v.cx = pKF->mK.template at<float>(0, 2); v.cy = pKF->mK.template at<float>(1, 2);
    return v;
  };
  v1 = view(pKF1);
  v2 = view(pKF2);
  const int N = (int)vpMatches1.size();
  const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches();
  pairs.clear();
  vnIndexEdge.clear();
  pairs.reserve(N);
  vnIndexEdge.reserve(N);
  for (int i = 0; i < N; i++) {   // :1436-1514
    if (!vpMatches1[i]) continue;
    MapPointT* pMP1 = vpMapPoints1[i];
    MapPointT* pMP2 = vpMatches1[i];
    const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (!pMP1 || !pMP2) continue;
    if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
    orbfe_optsim3_pair p;
    const cv::Mat P3D1w = pMP1->GetWorldPos(), P3D2w = pMP2->GetWorldPos();
    for (int r = 0; r < 3; r++) {
      p.Xw1[r] = P3D1w.template at<float>(r);
      p.Xw2[r] = P3D2w.template at<float>(r);
    }
    const auto& kpUn1 = pKF1->mvKeysUn[i];
    const auto& kpUn2 = pKF2->mvKeysUn[i2];
    p.obs1[0] = kpUn1.pt.x; p.obs1[1] = kpUn1.pt.y;
    p.obs2[0] = kpUn2.pt.x; p.obs2[1] = kpUn2.pt.y;
    p.inv_sigma2_1 = pKF1->mvInvLevelSigma2[kpUn1.octave];
    p.inv_sigma2_2 = pKF2->mvInvLevelSigma2[kpUn2.octave];
    pairs.push_back(p);
    vnIndexEdge.push_back((size_t)i);
  }
}

template <class KeyFrameT, class MapPointT, class Sim3T>
int OptimizeSim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, const float th2,
                 const bool bFixScale) {
  orbfe_sim3_view v1, v2;
  std::vector<orbfe_optsim3_pair> pairs;
  std::vector<size_t> vnIndexEdge;
  OptimizeSim3Marshal(pKF1, pKF2, vpMatches1, v1, v2, pairs, vnIndexEdge);
  float sRt[13];
  {
    const auto R = g2oS12.rotation().toRotationMatrix();
    const auto& t = g2oS12.translation();
    sRt[0] = (float)g2oS12.scale();
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) sRt[1 + 3 * r + c] = (float)R(r, c);
      sRt[10 + r] = (float)t[r];
    }
  }
  const int n = (int)pairs.size();
  orbfe_optsim3_result res;
  std::vector<uint8_t> bad((size_t)n, 0);
  const int rc = orbfe_optimize_sim3(&v1, &v2, pairs.data(), n, sRt, th2, bFixScale ? 1 : 0, &res, bad.data());
  if (rc != ORBFE_OK) {
    fprintf(stderr, "orbfe OptimizeSim3: %s (code %d)\n", orbfe_last_error(), rc);
    return 0;
  }
  for (int k = 0; k < n; k++)
    if (bad[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPointT*>(NULL);   // :1530, :1562
  if (res.n_pairs - res.n_bad < 10) return 0;                                // :1545, before g2oS12 is written
  std::decay_t<decltype(g2oS12.rotation().toRotationMatrix())> R;
  std::decay_t<decltype(g2oS12.translation())> t;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R(r, c) = (double)res.R[3 * r + c];
    t[r] = (double)res.t[r];
  }
  g2oS12 = Sim3T(R, t, (double)res.s);
  return res.n_inliers;
}

// What Optimizer::LocalBundleAdjustment collects and builds before it optimises (Optimizer.cc:440-644), as the library's arguments.
// Keyframe rows: lLocalKeyFrames in list order, then lFixedCameras; point rows: lLocalMapPoints in list order; edges in the order of
// the reference's addEdge calls, with the keyframe and the map point of each (vpEdgeKF*, vpMapPointEdge*).
template <class KeyFrameT, class MapPointT>
struct LocalBAProblem {
  std::list<KeyFrameT*> lLocalKeyFrames, lFixedCameras;
  std::list<MapPointT*> lLocalMapPoints;
  std::vector<float> poses, points;
  std::vector<uint8_t> fixed;
  std::vector<orbfe_lba_edge> edges;
  std::vector<KeyFrameT*> vpEdgeKF;
  std::vector<MapPointT*> vpMapPointEdge;
  orbfe_pose_camera cam;
};

template <class KeyFrameT, class MapPointT>
void LocalBundleAdjustmentMarshal(KeyFrameT* pKF, LocalBAProblem<KeyFrameT, MapPointT>& B) {
  // Local KeyFrames: first breadth search from the current keyframe (:440-451)
  B.lLocalKeyFrames.push_back(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  const std::vector<KeyFrameT*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
  for (int i = 0, iend = (int)vNeighKFs.size(); i < iend; i++) {
    KeyFrameT* pKFi = vNeighKFs[i];
    pKFi->mnBALocalForKF = pKF->mnId;
    if (!pKFi->isBad()) B.lLocalKeyFrames.push_back(pKFi);
  }
  // Local MapPoints seen in Local KeyFrames (:453-469)
  for (KeyFrameT* pKFi : B.lLocalKeyFrames) {
    const std::vector<MapPointT*> vpMPs = pKFi->GetMapPointMatches();
    for (MapPointT* pMP : vpMPs)
      if (pMP)
        if (!pMP->isBad())
          if (pMP->mnBALocalForKF != pKF->mnId) {
            B.lLocalMapPoints.push_back(pMP);
            pMP->mnBALocalForKF = pKF->mnId;
          }
  }
  // Fixed Keyframes: keyframes that see Local MapPoints but are not Local Keyframes (:471-490)
  for (MapPointT* pMP : B.lLocalMapPoints) {
    const auto observations = pMP->GetObservations();
    for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
      KeyFrameT* pKFi = mit->first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad()) B.lFixedCameras.push_back(pKFi);
      }
    }
  }
  // the vertices (:507-533, :564-569)
  std::map<KeyFrameT*, int32_t> row;
  auto add = [&B, &row](KeyFrameT* pKFi, bool fixed) {
    const cv::Mat T = pKFi->GetPose();
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) B.poses.push_back(T.template at<float>(r, c));
    row[pKFi] = (int32_t)B.fixed.size();
    B.fixed.push_back(fixed ? 1 : 0);
  };
  for (KeyFrameT* pKFi : B.lLocalKeyFrames) add(pKFi, pKFi->mnId == 0);
  for (KeyFrameT* pKFi : B.lFixedCameras) add(pKFi, true);
  memset(&B.cam, 0, sizeof(B.cam));
  B.cam.fx = pKF->fx;
  B.cam.fy = pKF->fy;
  B.cam.cx = pKF->cx;
  B.cam.cy = pKF->cy;
  B.cam.mbf = pKF->mbf;
  // the edges (:560-644)
  int32_t p = 0;
  for (MapPointT* pMP : B.lLocalMapPoints) {
    const cv::Mat Xw = pMP->GetWorldPos();
    for (int r = 0; r < 3; r++) B.points.push_back(Xw.template at<float>(r));
    const auto observations = pMP->GetObservations();
    for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
      KeyFrameT* pKFi = mit->first;
      if (pKFi->isBad()) continue;
      const auto it = row.find(pKFi);
      if (it == row.end()) continue;   // went bad while the sets were collected: the reference has no vertex for it either
      const auto& kpUn = pKFi->mvKeysUn[mit->second];
      orbfe_lba_edge e;
      e.kf = it->second;
      e.point = p;
      e.u = kpUn.pt.x;
      e.v = kpUn.pt.y;
      const float kp_ur = pKFi->mvuRight[mit->second];
      e.u_right = kp_ur < 0 ? -1.0f : kp_ur;
      e.inv_sigma2 = pKFi->mvInvLevelSigma2[kpUn.octave];
      B.edges.push_back(e);
      B.vpEdgeKF.push_back(pKFi);
      B.vpMapPointEdge.push_back(pMP);
    }
    p++;
  }
}

// The second half of LocalBundleAdjustment (:726-760) for a problem B and the library's outputs for it: under the map's mutex the
// erasures on both sides, SetPose of every local keyframe, SetWorldPos and UpdateNormalAndDepth of every local map point.
template <class KeyFrameT, class MapPointT, class MapT>
void LocalBundleAdjustmentApply(LocalBAProblem<KeyFrameT, MapPointT>& B, const float* poses_out, const float* points_out,
                                const uint8_t* erase, MapT* pMap) {
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  // vToErase: the monocular edges first, then the stereo ones (:700-736); the edge of a point that went bad is skipped
  const int n_edges = (int)B.edges.size();
  for (int pass = 0; pass < 2; pass++)
    for (int i = 0; i < n_edges; i++) {
      if ((B.edges[i].u_right < 0) != (pass == 0) || !(erase[i] & ORBFE_LBA_ERASE)) continue;
      MapPointT* pMPi = B.vpMapPointEdge[i];
      if (pMPi->isBad()) continue;
      B.vpEdgeKF[i]->EraseMapPointMatch(pMPi);
      pMPi->EraseObservation(B.vpEdgeKF[i]);
    }
  int k = 0;
  for (KeyFrameT* pKFi : B.lLocalKeyFrames) {
    cv::Mat pose = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) pose.template at<float>(r, c) = poses_out[(size_t)12 * k + 4 * r + c];
    pKFi->SetPose(pose);
    k++;
  }
  int p = 0;
  for (MapPointT* pMP : B.lLocalMapPoints) {
    cv::Mat X(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) X.template at<float>(r) = points_out[(size_t)3 * p + r];
    pMP->SetWorldPos(X);
    pMP->UpdateNormalAndDepth();
    p++;
  }
}

// void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap).  The stop flag is read before the one library
// call, not while it runs: an abort raised meanwhile takes effect once the call returns.  Errors (no device, a window
// beyond the library's limits) are logged and leave the map untouched, like a call whose stop flag is set on entry.
template <class KeyFrameT, class MapT>
void LocalBundleAdjustment(KeyFrameT* pKF, bool* pbStopFlag, MapT* pMap) {
  using MapPointT = std::remove_pointer_t<typename decltype(pKF->GetMapPointMatches())::value_type>;
  LocalBAProblem<KeyFrameT, MapPointT> B;
  LocalBundleAdjustmentMarshal(pKF, B);
  if (pbStopFlag)
    if (*pbStopFlag) return;   // :646
  const int n_kf = (int)B.fixed.size(), n_points = (int)(B.points.size() / 3), n_edges = (int)B.edges.size();
  std::vector<float> poses_out(B.poses.size()), points_out(B.points.size());
  std::vector<uint8_t> erase((size_t)n_edges, 0);
  orbfe_lba_result res;
  const int rc = orbfe_local_bundle_adjustment(&B.cam, B.poses.data(), B.fixed.data(), n_kf, B.points.data(), n_points, B.edges.data(),
                                               n_edges, 0, poses_out.data(), points_out.data(), erase.data(), &res);
  if (rc != ORBFE_OK) {
    fprintf(stderr, "orbfe LocalBundleAdjustment: %s (code %d)\n", orbfe_last_error(), rc);
    return;
  }
  LocalBundleAdjustmentApply(B, poses_out.data(), points_out.data(), erase.data(), pMap);
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
