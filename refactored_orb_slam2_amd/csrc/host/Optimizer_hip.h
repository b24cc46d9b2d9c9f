// Optimizer_hip.h -- host-side adapters that put ORB_SLAM2::Optimizer::PoseOptimization, Optimizer::OptimizeSim3,
// Optimizer::LocalBundleAdjustment and Optimizer::BundleAdjustment / GlobalBundleAdjustemnt on liborbfe.
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
//
// BundleAdjustment and GlobalBundleAdjustemnt (Optimizer.cc:43-231) are the adapters for orbfe_bundle_adjustment, with the
// reference's signatures, unit-tested by tests/cpp_ba.  A host that defines ORBFE_HOST_GLOBAL_BA_ACROSS_DEVICE before it includes
// this header gets, for a map beyond the ORBFE_LBA_MAX_* limits of that one-workgroup form, orbfe_global_bundle_adjustment instead
// of the refusal (unit-tested by tests/cpp_gba); the default keeps what every existing host sees.  Members used beyond the above:
//   KeyFrame: mTcwGBA, mnBAGlobalForKF
//   MapPoint: mPosGBA, mnBAGlobalForKF
//   Map:      GetAllKeyFrames(), GetAllMapPoints()
// AdjustAndScaleInitialMap is Tracking.cc:618-642 -- the adjustment of the two-keyframe map, the median depth, the reset rule and the
// rescale -- on orbfe_create_initial_map.  Members used beyond the above: KeyFrame::N, MapPoint::GetIndexInKeyFrame(KeyFrame*).
//
// OptimizeEssentialGraph (Optimizer.cc:1366, both forms) is the adapter for orbfe_essential_graph and orbfe_sim3_correct_points, with
// the reference's signature, split into a marshal and an apply half and unit-tested by tests/cpp/test_egraph_dropin.cpp.  A host that
// defines ORBFE_HOST_ESSENTIAL_GRAPH_ACROSS_DEVICE before it includes this header gets orbfe_essential_graph_grid -- one graph across
// the whole device, the same bytes -- for a graph beyond ORBFE_EG_MAX_ENVELOPE_BLOCKS instead of the refusal, and for every graph
// from the measured crossover kEssentialGraphGridFromBlocks on (unit-tested by tests/cpp_egraph_grid); the default keeps what every
// existing host sees.  Members used beyond the above:
//   KeyFrame: GetRotation(), GetTranslation(), GetParent(), hasChild(KeyFrame*), GetLoopEdges(), GetCovisiblesByWeight(int),
//             GetWeight(KeyFrame*)
//   MapPoint: mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame(), and what MapPoint_hip.h names
//   Map:      GetAllKeyFrames(), GetAllMapPoints()
//   Sim3:     rotation() with x() y() z() w(), translation(), scale(), the constructor (Matrix3, Vector3, double)
#pragma once
#include <stdio.h>
#include <string.h>

#include <list>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include <algorithm>
#include <set>
#include <utility>

#include "../../../include/orbfe.h"
#include "MapPoint_hip.h"

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

// What Optimizer::BundleAdjustment collects before it optimises (Optimizer.cc:70-181), as the library's arguments.  Keyframe rows:
// the keyframes of vpKFs that are not bad, in vector order; point rows: the map points of vpMP that are not bad, in vector order --
// included[p] == 0 for one without an edge, which the reference removes from the graph again; edges point by point in the order of
// the reference's addEdge calls, i.e. of the point's own std::map<KeyFrame*, size_t> (the library sorts them by keyframe row).
template <class KeyFrameT, class MapPointT>
struct GlobalBAProblem {
  std::vector<KeyFrameT*> vpKF;
  std::vector<MapPointT*> vpMP;
  std::vector<uint8_t> included;
  std::vector<float> poses, points;
  std::vector<uint8_t> fixed;
  std::vector<orbfe_lba_edge> edges;
  long unsigned int maxKFid = 0;
  orbfe_pose_camera cam;
};

template <class KeyFrameT, class MapPointT>
void BundleAdjustmentMarshal(const std::vector<KeyFrameT*>& vpKFs, const std::vector<MapPointT*>& vpMP,
                             GlobalBAProblem<KeyFrameT, MapPointT>& B) {
  memset(&B.cam, 0, sizeof(B.cam));
  std::map<KeyFrameT*, int32_t> row;
  for (KeyFrameT* pKF : vpKFs) {   // :74-85
    if (pKF->isBad()) continue;
    if (B.vpKF.empty()) {
      B.cam.fx = pKF->fx;
      B.cam.fy = pKF->fy;
      B.cam.cx = pKF->cx;
      B.cam.cy = pKF->cy;
      B.cam.mbf = pKF->mbf;
    }
    const cv::Mat T = pKF->GetPose();
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) B.poses.push_back(T.template at<float>(r, c));
    row[pKF] = (int32_t)B.vpKF.size();
    B.vpKF.push_back(pKF);
    B.fixed.push_back(pKF->mnId == 0 ? 1 : 0);
    if (pKF->mnId > B.maxKFid) B.maxKFid = pKF->mnId;
  }
  for (MapPointT* pMP : vpMP) {   // :91-181
    if (pMP->isBad()) continue;
    const int32_t p = (int32_t)B.vpMP.size();
    const cv::Mat Xw = pMP->GetWorldPos();
    for (int r = 0; r < 3; r++) B.points.push_back(Xw.template at<float>(r));
    B.vpMP.push_back(pMP);
    const auto observations = pMP->GetObservations();
    int nEdges = 0;
    for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
      KeyFrameT* pKF = mit->first;
      if (pKF->isBad() || pKF->mnId > B.maxKFid) continue;
      const auto it = row.find(pKF);
      if (it == row.end()) continue;   // not among vpKFs: the reference has no vertex for it
      nEdges++;
      const auto& kpUn = pKF->mvKeysUn[mit->second];
      orbfe_lba_edge e;
      e.kf = it->second;
      e.point = p;
      e.u = kpUn.pt.x;
      e.v = kpUn.pt.y;
      const float kp_ur = pKF->mvuRight[mit->second];
      e.u_right = kp_ur < 0 ? -1.0f : kp_ur;
      e.inv_sigma2 = pKF->mvInvLevelSigma2[kpUn.octave];
      B.edges.push_back(e);
    }
    B.included.push_back(nEdges > 0 ? 1 : 0);
  }
}

// "Recover optimized data" (:184-230) for a problem B and the library's outputs for it: into the map when nLoopKF == 0, beside it
// (mTcwGBA / mPosGBA / mnBAGlobalForKF) otherwise.  Every keyframe of the problem is written, the fixed one too, as the reference does
template <class KeyFrameT, class MapPointT>
void BundleAdjustmentApply(GlobalBAProblem<KeyFrameT, MapPointT>& B, const float* poses_out, const float* points_out,
                           const unsigned long nLoopKF) {
  for (size_t k = 0; k < B.vpKF.size(); k++) {
    KeyFrameT* pKF = B.vpKF[k];
    if (pKF->isBad()) continue;
    cv::Mat pose = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) pose.template at<float>(r, c) = poses_out[12 * k + 4 * r + c];
    if (nLoopKF == 0) {
      pKF->SetPose(pose);
    } else {
      pKF->mTcwGBA = pose;
      pKF->mnBAGlobalForKF = nLoopKF;
    }
  }
  for (size_t p = 0; p < B.vpMP.size(); p++) {
    if (!B.included[p]) continue;
    MapPointT* pMP = B.vpMP[p];
    if (pMP->isBad()) continue;
    cv::Mat X(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) X.template at<float>(r) = points_out[3 * p + r];
    if (nLoopKF == 0) {
      pMP->SetWorldPos(X);
      pMP->UpdateNormalAndDepth();
    } else {
      pMP->mPosGBA = X;
      pMP->mnBAGlobalForKF = nLoopKF;
    }
  }
}

// void Optimizer::BundleAdjustment(const vector<KeyFrame*>&, const vector<MapPoint*>&, int nIterations = 5, bool* pbStopFlag = NULL,
// const unsigned long nLoopKF = 0, const bool bRobust = true).  The stop flag is read before the one library call, not while it runs
// (INTEGRATION.md): found set on entry, nothing is done.  Errors (no device, a map beyond the library's limits) are logged and leave
// the map untouched.  There is no CPU fallback.
template <class KeyFrameT, class MapPointT>
void BundleAdjustment(const std::vector<KeyFrameT*>& vpKFs, const std::vector<MapPointT*>& vpMP, int nIterations = 5,
                      bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true) {
  if (pbStopFlag)
    if (*pbStopFlag) return;
  GlobalBAProblem<KeyFrameT, MapPointT> B;
  BundleAdjustmentMarshal(vpKFs, vpMP, B);
  const int n_kf = (int)B.vpKF.size(), n_points = (int)B.vpMP.size(), n_edges = (int)B.edges.size();
  std::vector<float> poses_out(B.poses.size()), points_out(B.points.size());
  orbfe_ba_result res;
  // Without ORBFE_HOST_GLOBAL_BA_ACROSS_DEVICE every map goes to the one-workgroup form, which refuses one beyond its limits, as
  // before (tests/cpp_ba pins that).  With it, a map within the ORBFE_LBA_MAX_* limits still goes there and any other to the form
  // that spreads one problem over the device (profiles/global_bundle_adjustment.md has both on one scene at the limit)
#ifdef ORBFE_HOST_GLOBAL_BA_ACROSS_DEVICE
  int n_free = 0;
  for (const uint8_t f : B.fixed) n_free += f ? 0 : 1;
  const bool one_workgroup = n_free <= ORBFE_LBA_MAX_FREE && n_kf <= ORBFE_LBA_MAX_KEYFRAMES && n_points <= ORBFE_LBA_MAX_POINTS &&
                             n_edges <= ORBFE_LBA_MAX_EDGES;
#else
  const bool one_workgroup = true;
#endif
  const int rc = (one_workgroup ? orbfe_bundle_adjustment : orbfe_global_bundle_adjustment)(
      &B.cam, B.poses.data(), B.fixed.data(), n_kf, B.points.data(), n_points, B.edges.data(), n_edges, nIterations,
      bRobust ? ORBFE_BA_ROBUST : 0, poses_out.data(), points_out.data(), &res);
  if (rc != ORBFE_OK) {
    fprintf(stderr, "orbfe BundleAdjustment: %s (code %d)\n", orbfe_last_error(), rc);
    return;
  }
  BundleAdjustmentApply(B, poses_out.data(), points_out.data(), nLoopKF);
}

// void Optimizer::GlobalBundleAdjustemnt(Map* pMap, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0,
// const bool bRobust = true)
template <class MapT>
void GlobalBundleAdjustemnt(MapT* pMap, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0,
                            const bool bRobust = true) {
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMP = pMap->GetAllMapPoints();
  BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}

// Tracking.cc:618-642 for the two keyframes of CreateInitialMapMonocular, after the map points were created (:584-612): the global
// bundle adjustment of nIterations, the median depth of the scene in pKFini, the reset rule and the rescale, in ONE library call
// (orbfe_create_initial_map; nothing of it is computed here).  Returns false where Tracking resets ("Wrong initialization"); the
// poses and points are then the adjustment's, as in the reference.  The adjustment's values are written with SetPose / SetWorldPos +
// UpdateNormalAndDepth, the rescaled ones with SetPose / SetWorldPos alone, as :636-642 do.  Errors are logged, leave the map
// untouched and return false.  *result (may be NULL) receives the library's record.
template <class KeyFrameT>
bool AdjustAndScaleInitialMap(KeyFrameT* pKFini, KeyFrameT* pKFcur, int nIterations = 20, orbfe_initial_map_result* result = NULL) {
  using MapPointT = std::remove_pointer_t<typename decltype(pKFini->GetMapPointMatches())::value_type>;
  const std::vector<MapPointT*> vpMP = pKFini->GetMapPointMatches();
  const int n1 = pKFini->N, n2 = pKFcur->N, nw = (n1 + 63) / 64;
  std::vector<float> keys1((size_t)2 * n1), keys2((size_t)2 * n2), P3D((size_t)3 * n1, 0.0f);
  std::vector<int32_t> oct1(n1), oct2(n2), matches12(n1, -1);
  std::vector<uint64_t> tri(nw > 0 ? nw : 1, 0);
  for (int i = 0; i < n1; i++) {
    keys1[2 * i] = pKFini->mvKeysUn[i].pt.x;
    keys1[2 * i + 1] = pKFini->mvKeysUn[i].pt.y;
    oct1[i] = pKFini->mvKeysUn[i].octave;
  }
  for (int j = 0; j < n2; j++) {
    keys2[2 * j] = pKFcur->mvKeysUn[j].pt.x;
    keys2[2 * j + 1] = pKFcur->mvKeysUn[j].pt.y;
    oct2[j] = pKFcur->mvKeysUn[j].octave;
  }
  for (int i = 0; i < n1 && i < (int)vpMP.size(); i++) {
    MapPointT* pMP = vpMP[i];
    if (!pMP) continue;
    const int j = pMP->GetIndexInKeyFrame(pKFcur);
    if (j < 0) continue;
    matches12[i] = j;
    tri[i >> 6] |= 1ull << (i & 63);
    const cv::Mat Xw = pMP->GetWorldPos();
    for (int r = 0; r < 3; r++) P3D[3 * i + r] = Xw.template at<float>(r);
  }
  orbfe_pose_camera cam;
  memset(&cam, 0, sizeof(cam));
  cam.fx = pKFini->fx;
  cam.fy = pKFini->fy;
  cam.cx = pKFini->cx;
  cam.cy = pKFini->cy;
  cam.mbf = pKFini->mbf;
  cam.n_levels = (int32_t)pKFini->mvInvLevelSigma2.size();
  for (int l = 0; l < cam.n_levels && l < ORBFE_MAX_LEVELS; l++) cam.inv_level_sigma2[l] = pKFini->mvInvLevelSigma2[l];
  orbfe_init_result init;
  memset(&init, 0, sizeof(init));
  float pose1[12];
  const cv::Mat T1 = pKFini->GetPose(), T2 = pKFcur->GetPose();
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 4; c++) pose1[4 * r + c] = T1.template at<float>(r, c);
    for (int c = 0; c < 3; c++) init.R21[3 * r + c] = T2.template at<float>(r, c);
    init.t21[r] = T2.template at<float>(r, 3);
  }
  std::vector<float> points((size_t)3 * n1), points_ba((size_t)3 * n1);
  std::vector<int32_t> index(n1 > 0 ? n1 : 1);
  float poses[24], poses_ba[24];
  orbfe_initial_map_result res;
  const int rc = orbfe_create_initial_map(&cam, keys1.data(), n1, keys2.data(), n2, matches12.data(), P3D.data(), tri.data(), &init, oct1.data(),
                                          oct2.data(), pose1, nIterations, 2, 100, poses, points.data(), index.data(), poses_ba,
                                          points_ba.data(), &res);
  if (rc != ORBFE_OK) {
    fprintf(stderr, "orbfe AdjustAndScaleInitialMap: %s (code %d)\n", orbfe_last_error(), rc);
    return false;
  }
  if (result) *result = res;
  auto pose_of = [](const float* T) {
    cv::Mat pose = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) pose.template at<float>(r, c) = T[4 * r + c];
    return pose;
  };
  auto point_of = [](const float* X) {
    cv::Mat x(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) x.template at<float>(r) = X[r];
    return x;
  };
  if (res.ba.rounds > 0) {   // GlobalBundleAdjustemnt(mpMap, 20)
    pKFini->SetPose(pose_of(poses_ba));
    pKFcur->SetPose(pose_of(poses_ba + 12));
    for (int k = 0; k < res.n_points; k++) {
      MapPointT* pMP = vpMP[index[k]];
      pMP->SetWorldPos(point_of(points_ba.data() + 3 * index[k]));
      pMP->UpdateNormalAndDepth();
    }
  }
  if (!res.success) return false;   // :623
  pKFcur->SetPose(pose_of(poses + 12));   // :630-633
  for (int k = 0; k < res.n_points; k++) vpMP[index[k]]->SetWorldPos(point_of(points.data() + 3 * index[k]));   // :636-642
  return true;
}

// g2o::Sim3's own fields into the library's record: a copy, never a conversion
template <class Sim3T>
orbfe_eg_sim3 EssentialGraphRecord(const Sim3T& S) {
  orbfe_eg_sim3 r;
  r.q[0] = S.rotation().x();
  r.q[1] = S.rotation().y();
  r.q[2] = S.rotation().z();
  r.q[3] = S.rotation().w();
  for (int k = 0; k < 3; k++) r.t[k] = S.translation()[k];
  r.s = S.scale();
  return r;
}

// Sim3(Rcw, tcw, 1.0) of a float pose by the caller's own Sim3 type (Optimizer.cc:813-818, LoopClosing.cc:435-438)
template <class Sim3T>
Sim3T EssentialGraphSim3(const cv::Mat& R, const cv::Mat& t) {
  std::decay_t<decltype(std::declval<Sim3T>().rotation().toRotationMatrix())> Rd;
  std::decay_t<decltype(std::declval<Sim3T>().translation())> td;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Rd(r, c) = (double)R.template at<float>(r, c);
    td[r] = (double)t.template at<float>(r);
  }
  return Sim3T(Rd, td, 1.0);
}

// What Optimizer::OptimizeEssentialGraph builds before it optimises (Optimizer.cc:787-985, :1083-1301), as the library's arguments.
// Vertex rows: the keyframes that are not bad, ascending by mnId -- the elimination order of the library's solve; edges in the order of
// the reference's addEdge calls over that keyframe order; point rows: GetAllMapPoints() in its order, ref = the vertex row of the
// keyframe the point is corrected through (:1022-1028), -1 for a bad point.
template <class KeyFrameT, class MapPointT>
struct EssentialGraphProblem {
  std::vector<KeyFrameT*> vpKFs;
  std::vector<orbfe_eg_vertex> vertices;
  std::vector<orbfe_eg_edge> edges;
  std::vector<MapPointT*> vpMPs;
  std::vector<float> points;
  std::vector<int32_t> ref;
};

template <class MapT, class KeyFrameT, class MapPointT, class PoseMapT, class ConnectionsT>
void OptimizeEssentialGraphMarshal(MapT* pMap, KeyFrameT* pLoopKF, KeyFrameT* pCurKF, const PoseMapT& NonCorrectedSim3,
                                   const PoseMapT& CorrectedSim3, const ConnectionsT& LoopConnections,
                                   EssentialGraphProblem<KeyFrameT, MapPointT>& B) {
  typedef typename PoseMapT::mapped_type Sim3T;
  const int minFeat = 100;
  for (KeyFrameT* pKF : pMap->GetAllKeyFrames())
    if (!pKF->isBad()) B.vpKFs.push_back(pKF);
  std::sort(B.vpKFs.begin(), B.vpKFs.end(), [](KeyFrameT* a, KeyFrameT* b) { return a->mnId < b->mnId; });
  std::map<KeyFrameT*, int32_t> row;
  std::map<long unsigned int, int32_t> row_of_id;
  // Set KeyFrame vertices (:799-831)
  for (KeyFrameT* pKF : B.vpKFs) {
    orbfe_eg_vertex v;
    memset(&v, 0, sizeof(v));
    const auto it = CorrectedSim3.find(pKF);
    v.Scw = it != CorrectedSim3.end() ? EssentialGraphRecord(it->second)
                                      : EssentialGraphRecord(EssentialGraphSim3<Sim3T>(pKF->GetRotation(), pKF->GetTranslation()));
    const auto itn = NonCorrectedSim3.find(pKF);
    v.Snc = itn != NonCorrectedSim3.end() ? EssentialGraphRecord(itn->second) : v.Scw;
    v.fixed = pKF == pLoopKF ? 1 : 0;
    row[pKF] = row_of_id[pKF->mnId] = (int32_t)B.vertices.size();
    B.vertices.push_back(v);
  }
  // an edge one of whose keyframes has no vertex is not added by g2o either
  auto add = [&B, &row](KeyFrameT* a, KeyFrameT* b, uint32_t kind) {
    const auto ia = row.find(a), ib = row.find(b);
    if (ia == row.end() || ib == row.end() || ia->second == ib->second) return;
    orbfe_eg_edge e;
    e.i = ia->second;
    e.j = ib->second;
    e.kind = kind;
    B.edges.push_back(e);
  };
  std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
  // Set Loop edges (:839-873)
  for (auto mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
    KeyFrameT* pKF = mit->first;
    const long unsigned int nIDi = pKF->mnId;
    for (KeyFrameT* pKFj : mit->second) {
      const long unsigned int nIDj = pKFj->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat) continue;
      add(pKF, pKFj, ORBFE_EG_LOOP_CONNECTION);
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  // Set normal edges (:876-985)
  for (KeyFrameT* pKF : B.vpKFs) {
    KeyFrameT* pParentKF = pKF->GetParent();
    if (pParentKF) add(pKF, pParentKF, ORBFE_EG_NORMAL);   // Spanning tree edge
    const auto sLoopEdges = pKF->GetLoopEdges();
    for (KeyFrameT* pLKF : sLoopEdges)
      if (pLKF->mnId < pKF->mnId) add(pKF, pLKF, ORBFE_EG_NORMAL);
    const std::vector<KeyFrameT*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (KeyFrameT* pKFn : vpConnectedKFs)
      if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn))
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
          add(pKF, pKFn, ORBFE_EG_NORMAL);
        }
  }
  // the point table (:1016-1034)
  B.vpMPs = pMap->GetAllMapPoints();
  B.points.assign(3 * B.vpMPs.size(), 0.0f);
  B.ref.assign(B.vpMPs.size(), -1);
  for (size_t i = 0; i < B.vpMPs.size(); i++) {
    MapPointT* pMP = B.vpMPs[i];
    if (!pMP || pMP->isBad()) continue;
    const long unsigned int nIDr = pMP->mnCorrectedByKF == pCurKF->mnId ? pMP->mnCorrectedReference : pMP->GetReferenceKeyFrame()->mnId;
    const auto it = row_of_id.find(nIDr);
    if (it == row_of_id.end()) continue;   // the reference keyframe has no vertex: the point is left alone
    B.ref[i] = it->second;
    const cv::Mat P3Dw = pMP->GetWorldPos();
    for (int r = 0; r < 3; r++) B.points[3 * i + r] = P3Dw.template at<float>(r);
  }
}

// The second half of OptimizeEssentialGraph (:991-1042, :1307-1361) for a problem B and the library's outputs for it: under the map's
// mutex SetPose of every keyframe with a vertex, SetWorldPos of every point with a row, and their UpdateNormalAndDepth in ONE batch
// (MapPoint_hip.h) instead of per point.
template <class KeyFrameT, class MapPointT, class MapT>
void OptimizeEssentialGraphApply(EssentialGraphProblem<KeyFrameT, MapPointT>& B, const float* poses_out, const float* points_out, MapT* pMap) {
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  for (size_t k = 0; k < B.vpKFs.size(); k++) {
    cv::Mat Tiw = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) Tiw.template at<float>(r, c) = poses_out[12 * k + 4 * r + c];
    B.vpKFs[k]->SetPose(Tiw);
  }
  std::vector<MapPointT*> moved;
  for (size_t i = 0; i < B.vpMPs.size(); i++) {
    if (B.ref[i] < 0) continue;
    cv::Mat X(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) X.template at<float>(r) = points_out[3 * i + r];
    B.vpMPs[i]->SetWorldPos(X);
    moved.push_back(B.vpMPs[i]);
  }
  UpdateNormalAndDepth(moved);
}

// The envelope blocks from which OptimizeEssentialGraph, compiled with ORBFE_HOST_ESSENTIAL_GRAPH_ACROSS_DEVICE, hands a graph to
// orbfe_essential_graph_grid: the measured crossover of the two forms (profiles/essential_graph.md; one MI355X, tools/egraph_rate.py
// on graphs of band 20, Sim3 / SE3, one workgroup against across the device).  At 66 blocks (12 keyframes) the one-workgroup form
// is the faster one, 3.5 / 1.6 ms against 3.9 / 2.8 ms; at 190 blocks (20 keyframes) the form across the device is, 6.0 / 4.3 ms
// against 9.3 / 5.0 ms, and it stays so at every larger size measured (609 blocks: 2.5 / 2.1 times; 41 769 blocks: 4.0 / 3.6 times).
constexpr int64_t kEssentialGraphGridFromBlocks = 190;

// Whether the form across the device is the one for problem B: by its envelope (orbfe_essential_graph_envelope_blocks) against the
// constant above.  Needs no device.
template <class KeyFrameT, class MapPointT>
bool EssentialGraphAcrossDevice(const EssentialGraphProblem<KeyFrameT, MapPointT>& B) {
  std::vector<uint8_t> fixed(B.vertices.size());
  for (size_t k = 0; k < B.vertices.size(); k++) fixed[k] = B.vertices[k].fixed ? 1 : 0;
  int64_t blocks = 0;
  if (orbfe_essential_graph_envelope_blocks((int)B.vertices.size(), fixed.data(), B.edges.data(), (int)B.edges.size(), &blocks) != ORBFE_OK)
    return false;
  return blocks >= kEssentialGraphGridFromBlocks;
}

// void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose&
// NonCorrectedSim3, const LoopClosing::KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections, const
// bool& bFixScale).  Two library calls: the graph, then the map correction.  Errors (no device, a graph beyond the library's limits,
// a scale beyond 1e-3 of 1 with bFixScale -- where the reference throws) are logged and leave the map untouched.
template <class MapT, class KeyFrameT, class PoseMapT, class ConnectionsT>
void OptimizeEssentialGraph(MapT* pMap, KeyFrameT* pLoopKF, KeyFrameT* pCurKF, const PoseMapT& NonCorrectedSim3,
                            const PoseMapT& CorrectedSim3, const ConnectionsT& LoopConnections, const bool& bFixScale) {
  using MapPointT = std::remove_pointer_t<typename decltype(pMap->GetAllMapPoints())::value_type>;
  EssentialGraphProblem<KeyFrameT, MapPointT> B;
  OptimizeEssentialGraphMarshal(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, B);
  const int n_kf = (int)B.vertices.size(), n_pt = (int)B.vpMPs.size();
  std::vector<orbfe_eg_sim3> sim3_out((size_t)n_kf), vScw((size_t)n_kf);
  std::vector<float> poses_out((size_t)12 * n_kf), points_out((size_t)3 * n_pt);
  orbfe_eg_result res;
  const int n_edges = (int)B.edges.size(), flags = bFixScale ? ORBFE_EG_FIX_SCALE : 0;
  // Without ORBFE_HOST_ESSENTIAL_GRAPH_ACROSS_DEVICE every graph goes to the one-workgroup form, which refuses one beyond its envelope
  // limit, as every existing host sees.  With it, the form across the device takes such a graph -- and every graph from the crossover
  // on: the two forms give the same bytes, so the choice is only a matter of time.  A graph whose envelope cannot be counted (a limit
  // broken) goes to the one-workgroup form, which reports it.
  bool across_device = false;
#ifdef ORBFE_HOST_ESSENTIAL_GRAPH_ACROSS_DEVICE
  across_device = EssentialGraphAcrossDevice(B);
#endif
  int rc = across_device ? orbfe_essential_graph_grid(B.vertices.data(), n_kf, B.edges.data(), n_edges, flags, sim3_out.data(),
                                                      poses_out.data(), &res)
                         : orbfe_essential_graph(B.vertices.data(), n_kf, B.edges.data(), n_edges, flags, sim3_out.data(),
                                                 poses_out.data(), &res);
  if (rc == ORBFE_OK) {
    for (int k = 0; k < n_kf; k++) vScw[k] = B.vertices[k].Scw;
    rc = orbfe_sim3_correct_points(B.points.data(), n_pt, B.ref.data(), vScw.data(), sim3_out.data(), n_kf, points_out.data());
  }
  if (rc != ORBFE_OK) {
    fprintf(stderr, "orbfe OptimizeEssentialGraph: %s (code %d)\n", orbfe_last_error(), rc);
    return;
  }
  OptimizeEssentialGraphApply(B, poses_out.data(), points_out.data(), pMap);
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
