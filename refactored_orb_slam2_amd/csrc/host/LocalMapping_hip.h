// LocalMapping_hip.h -- host-side adapter that puts the neighbour loop of ORB_SLAM2::LocalMapping::CreateNewMapPoints on liborbfe.
//
// The reference's function (Source/Libraries/ORB_SLAM2/src/LocalMapping.cc:185-423) walks the covisible neighbours of the current
// keyframe: baseline gate, ComputeF12, SearchForTriangulation, then per match the triangulation, its gates and the creation of the
// MapPoint.  This template marshals what the loop reads into ONE orbfe_create_new_map_points call (include/orbfe.h) and hands back,
// per neighbour, the accepted (idx1, idx2, x3D) in the reference's order; the caller runs the reference's bookkeeping on them (new
// MapPoint, AddObservation, AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth, mlpRecentAddedMapPoints), which has
// to happen on the SLAM objects.  ComputeF12 and the epipole stay the caller's, as for SearchForTriangulation: one callback per
// neighbour that passes the baseline gate.  A template over the KeyFrame type so that it compiles (and is unit-tested, tests/cpp_mapping) without the reference
// tree; INTEGRATION.md shows the body a maintainer replaces.
//
// Members used (same names as the reference):
//   KeyFrame: N, mvKeysUn, mvuRight, mvDepth, mDescriptors, mFeatVec, GetMapPoint(i), GetRotation(), GetTranslation(),
//             GetCameraCenter(), fx, fy, cx, cy, invfx, invfy, mb, mbf, mvScaleFactors, mvLevelSigma2, ComputeSceneMedianDepth(2)
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <type_traits>
#include <vector>

#include "../../../include/orbfe.h"
#include "MapPoint_hip.h"
#include "ORBmatcher_hip.h"

namespace ORB_SLAM2 {
namespace orbfe_host {

struct NewMapPoint {   // one accepted pair: what `new MapPoint(x3D, mpCurrentKeyFrame, mpMap)` and the two AddObservation calls need
  size_t idx1, idx2;
  float x3D[3];
  float normal[3], min_distance, max_distance;   // what UpdateNormalAndDepth will compute for it
};
struct NeighborResult {
  bool skipped = false;                // the baseline gate (:226-235) skipped this neighbour
  int nmatches = 0;                    // vMatchedIndices.size()
  std::vector<NewMapPoint> points;     // ascending idx1 = the reference's order
};

template <class KeyFrameT>
inline orbfe_tri_view MakeTriView(KeyFrameT* pKF) {
  orbfe_tri_view v;
  memset(&v, 0, sizeof(v));
  const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) v.Rcw[3 * r + c] = R.template at<float>(r, c);
    v.tcw[r] = t.template at<float>(r);
    v.Ow[r] = O.template at<float>(r);
  }
  v.fx = pKF->fx; v.fy = pKF->fy; v.cx = pKF->cx; v.cy = pKF->cy;
  v.invfx = pKF->invfx; v.invfy = pKF->invfy; v.mb = pKF->mb; v.mbf = pKF->mbf;
  v.n_levels = (int32_t)pKF->mvScaleFactors.size();
  for (size_t l = 0; l < pKF->mvScaleFactors.size() && l < ORBFE_MAX_LEVELS; l++) {
    v.scale_factors[l] = pKF->mvScaleFactors[l];
    v.level_sigma2[l] = pKF->mvLevelSigma2[l];
  }
  return v;
}

// The baseline gate of :221-235, as the library applies it (float differences, cv::norm in double, rounded once)
inline bool BaselineTooShort(const orbfe_tri_view& v1, const orbfe_tri_view& v2, bool bMonocular, float medianDepthKF2) {
  double s = 0.0;
  for (int r = 0; r < 3; r++) {
    const float d = v2.Ow[r] - v1.Ow[r];
    s += (double)d * (double)d;
  }
  const float baseline = (float)sqrt(s);
  if (!bMonocular) return baseline < v2.mb;
  const float ratioBaselineDepth = baseline / medianDepthKF2;
  return ratioBaselineDepth < 0.01;
}

// The loop of :215-422 for pKF1 = mpCurrentKeyFrame and vpNeighKFs.  epipolarOf(pKF1, pKF2, F12, &ex, &ey) fills the nine row-major
// floats of ComputeF12(pKF1, pKF2) and the epipole of ORBmatcher.cc:622-630.  Returns nnew, or -1 after logging an error (no
// device, a keyframe beyond the library's limits) with `out` empty.
template <class KeyFrameT, class EpipolarFn>
int CreateNewMapPoints(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, bool bMonocular, EpipolarFn epipolarOf,
                       std::vector<NeighborResult>& out, bool checkOrientation = false) {
  static_assert(sizeof(pKF1->mvKeysUn[0]) == sizeof(orbfe_keypoint), "cv::KeyPoint layout");
  out.clear();
  const int K = (int)vpNeighKFs.size(), n1 = pKF1->N;
  std::vector<orbfe_featvec_node> nodes1;
  std::vector<int32_t> idx1;
  FlattenFeatureVector(pKF1->mFeatVec, nodes1, idx1);
  std::vector<uint8_t> has1((size_t)(n1 > 0 ? n1 : 1));
  for (int i = 0; i < n1; i++) has1[i] = pKF1->GetMapPoint((size_t)i) != nullptr;
  const orbfe_tri_view view1 = MakeTriView(pKF1);
  std::vector<orbfe_tri_neighbor> nb((size_t)K);
  std::vector<std::vector<orbfe_featvec_node>> nodes2((size_t)K);
  std::vector<std::vector<int32_t>> idx2((size_t)K);
  std::vector<std::vector<uint8_t>> has2((size_t)K);
  for (int k = 0; k < K; k++) {
    KeyFrameT* pKF2 = vpNeighKFs[(size_t)k];
    orbfe_tri_neighbor& N = nb[(size_t)k];
    memset(&N, 0, sizeof(N));
    FlattenFeatureVector(pKF2->mFeatVec, nodes2[k], idx2[k]);
    has2[k].resize((size_t)(pKF2->N > 0 ? pKF2->N : 1));
    for (int i = 0; i < pKF2->N; i++) has2[k][i] = pKF2->GetMapPoint((size_t)i) != nullptr;
    N.keys = reinterpret_cast<const orbfe_keypoint*>(pKF2->mvKeysUn.data());
    N.desc = pKF2->mDescriptors.ptr(0);
    N.u_right = pKF2->mvuRight.empty() ? nullptr : pKF2->mvuRight.data();
    N.depth = pKF2->mvuRight.empty() ? nullptr : pKF2->mvDepth.data();
    N.has_mp = has2[k].data();
    N.nodes = nodes2[k].data();
    N.idx = idx2[k].data();
    N.n = pKF2->N;
    N.n_nodes = (int32_t)nodes2[k].size();
    N.view = MakeTriView(pKF2);
    N.median_depth = bMonocular ? pKF2->ComputeSceneMedianDepth(2) : 0.0f;
    // the reference gates before ComputeF12 (:221-238): a neighbour the library will skip costs no fundamental matrix (its
    // epipolar record stays zero and is never read)
    if (BaselineTooShort(view1, N.view, bMonocular, N.median_depth)) continue;
    epipolarOf(pKF1, pKF2, N.ep.F12, &N.ep.ex, &N.ep.ey);
    memcpy(N.ep.scale_factors, N.view.scale_factors, sizeof(N.ep.scale_factors));
    memcpy(N.ep.level_sigma2, N.view.level_sigma2, sizeof(N.ep.level_sigma2));
  }
  std::vector<orbfe_new_point> pts((size_t)K * (size_t)n1 + 1);
  std::vector<int32_t> nm((size_t)K + 1), nn((size_t)K + 1);
  const int rc = orbfe_create_new_map_points(
      reinterpret_cast<const orbfe_keypoint*>(pKF1->mvKeysUn.data()), pKF1->mDescriptors.ptr(0),
      pKF1->mvuRight.empty() ? nullptr : pKF1->mvuRight.data(), pKF1->mvuRight.empty() ? nullptr : pKF1->mvDepth.data(), has1.data(), n1,
      nodes1.data(), (int)nodes1.size(), idx1.data(), &view1, nb.data(), K, bMonocular ? 1 : 0, 0, checkOrientation ? 1 : 0, pts.data(),
      nm.data(), nn.data());
  if (rc != ORBFE_OK) {
    fprintf(stderr, "LocalMapping::CreateNewMapPoints: liborbfe error %d: %s\n", rc, orbfe_last_error());
    return -1;
  }
  // has1 now also marks the accepted features; it is dropped: the caller's AddMapPoint calls put the same facts into pKF1
  int nnew = 0;
  out.resize((size_t)K);
  for (int k = 0; k < K; k++) {
    NeighborResult& R = out[(size_t)k];
    R.skipped = nm[k] < 0;
    R.nmatches = nm[k] < 0 ? 0 : nm[k];
    for (int i = 0; i < n1; i++) {
      const orbfe_new_point& p = pts[(size_t)k * n1 + i];
      if (p.code != ORBFE_TRI_OK) continue;
      NewMapPoint m;
      m.idx1 = (size_t)i;
      m.idx2 = (size_t)p.idx2;
      memcpy(m.x3D, p.pos, sizeof(m.x3D));
      memcpy(m.normal, p.normal, sizeof(m.normal));
      m.min_distance = p.min_distance;
      m.max_distance = p.max_distance;
      R.points.push_back(m);
      nnew++;
    }
  }
  return nnew;
}

// ---- LocalMapping::SearchInNeighbors (Source/Libraries/ORB_SLAM2/src/LocalMapping.cc:425-509) with all ORBmatcher::Fuse calls of the
// forward loop in ONE batched search (include/orbfe.h: orbfe_fuse_batch_*).  The K calls of the reference depend on each other only
// through the map, and the one search input a MapPoint::Replace changes is the survivor's descriptor: every row (target, point) is
// searched once, the targets are replayed in order on the real objects with the loop of ORBmatcher::Fuse (:870-884), and before the
// replay enters the next target the points whose GetDescriptor() bytes changed around a Replace are searched again in the targets
// still ahead.  The result is the reference's sequence of AddObservation / AddMapPoint / Replace calls in 2 + (boundaries with a
// changed descriptor) device round trips instead of K + 1.
//
// Members used beyond those of CreateNewMapPoints (same names as the reference):
//   KeyFrame: mnId, mnFuseTargetForKF, isBad(), GetBestCovisibilityKeyFrames(n), GetMapPointMatches(), AddMapPoint(), UpdateConnections(),
//             mnMinX .. mnMaxY, mfLogScaleFactor, mnScaleLevels, mvInvLevelSigma2
//   MapPoint: mnFuseCandidateForKF, isBad(), IsInKeyFrame(), Observations(), Replace(), AddObservation(), GetWorldPos(), GetNormal(),
//             GetDescriptor(), mfMinDistance / mfMaxDistance (protected: read through a pointer to member formed in a derived class)
template <class MapPointT>
struct FusePointAccess : public MapPointT {   // never instantiated
  static float MapPointT::*MinDistance() { return &FusePointAccess::mfMinDistance; }
  static float MapPointT::*MaxDistance() { return &FusePointAccess::mfMaxDistance; }
};

template <class MapPointT>
inline void FillFusePoint(orbfe_kf_point& e, MapPointT* pMP) {
  memset(&e, 0, sizeof(e));
  const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal(), d = pMP->GetDescriptor();
  for (int r = 0; r < 3; r++) { e.pos[r] = P.template at<float>(r); e.normal[r] = Pn.template at<float>(r); }
  e.min_distance = pMP->*FusePointAccess<MapPointT>::MinDistance();
  e.max_distance = pMP->*FusePointAccess<MapPointT>::MaxDistance();
  memcpy(e.desc, d.ptr(0), 32);
}

template <class KeyFrameT>
inline void FillFuseTarget(KeyFrameT* pKF, float th, orbfe_frame_view& v, orbfe_kf_camera& cam, float* inv_level_sigma2) {
  static_assert(sizeof(pKF->mvKeysUn[0]) == sizeof(orbfe_keypoint), "cv::KeyPoint layout");
  v.n = pKF->N;
  v.keys_un = reinterpret_cast<const orbfe_keypoint*>(pKF->mvKeysUn.data());
  v.desc = pKF->mDescriptors.ptr(0);
  v.u_right = pKF->mvuRight.empty() ? nullptr : pKF->mvuRight.data();
  v.min_x = (float)pKF->mnMinX; v.max_x = (float)pKF->mnMaxX; v.min_y = (float)pKF->mnMinY; v.max_y = (float)pKF->mnMaxY;
  memset(&cam, 0, sizeof(cam));
  const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) cam.R[3 * r + c] = R.template at<float>(r, c);
    cam.t[r] = t.template at<float>(r);
    cam.Ow[r] = O.template at<float>(r);
  }
  cam.fx = pKF->fx; cam.fy = pKF->fy; cam.cx = pKF->cx; cam.cy = pKF->cy; cam.mbf = pKF->mbf;
  cam.min_x = v.min_x; cam.max_x = v.max_x; cam.min_y = v.min_y; cam.max_y = v.max_y;
  cam.log_scale_factor = pKF->mfLogScaleFactor;
  cam.n_levels = pKF->mnScaleLevels;
  cam.th = th;
  for (int l = 0; l < ORBFE_MAX_LEVELS; l++) {
    const bool in = l < pKF->mnScaleLevels;
    cam.scale_factors[l] = in && l < (int)pKF->mvScaleFactors.size() ? pKF->mvScaleFactors[l] : 0.f;
    inv_level_sigma2[l] = in && l < (int)pKF->mvInvLevelSigma2.size() ? pKF->mvInvLevelSigma2[l] : 0.f;
  }
}

// One fuse batch over `targets`, searched for `points`: what the forward pass (K targets) and the reverse pass (one) both open.
template <class KeyFrameT, class MapPointT>
struct FuseBatchRun {
  orbfe_fuse_batch* batch = nullptr;
  std::vector<orbfe_kf_point> rec;
  std::vector<orbfe_kf_result> rows;
  int K = 0, n = 0;
  ~FuseBatchRun() { orbfe_fuse_batch_destroy(batch); }

  bool Fail(const char* what, int rc) {
    fprintf(stderr, "LocalMapping::SearchInNeighbors: %s: liborbfe error %d: %s\n", what, rc, orbfe_last_error());
    return false;
  }
  bool Open(const std::vector<KeyFrameT*>& targets, const std::vector<MapPointT*>& points, float th) {
    K = (int)targets.size(); n = (int)points.size();
    std::vector<orbfe_frame_view> views((size_t)K);
    std::vector<orbfe_kf_camera> cams((size_t)K);
    std::vector<float> inv((size_t)K * ORBFE_MAX_LEVELS + 1);
    for (int k = 0; k < K; k++) FillFuseTarget(targets[(size_t)k], th, views[(size_t)k], cams[(size_t)k], &inv[(size_t)k * ORBFE_MAX_LEVELS]);
    int rc = orbfe_fuse_batch_create(K, views.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &batch);
    if (rc != ORBFE_OK) return Fail("orbfe_fuse_batch_create", rc);
    rec.resize((size_t)n + 1);
    std::vector<uint8_t> skip((size_t)K * (size_t)n + 1, 0);
    for (int i = 0; i < n; i++) {
      MapPointT* pMP = points[(size_t)i];
      if (!pMP || pMP->isBad()) { memset(&rec[(size_t)i], 0, sizeof(orbfe_kf_point)); rec[(size_t)i].skip = 1; }
      else FillFusePoint(rec[(size_t)i], pMP);
      for (int k = 0; k < K; k++) skip[(size_t)k * n + i] = !pMP || pMP->isBad() || pMP->IsInKeyFrame(targets[(size_t)k]);   // :787
    }
    rows.assign((size_t)K * (size_t)n + 1, orbfe_kf_result());
    rc = orbfe_fuse_batch_search(batch, rec.data(), n, nullptr, 0, 0, skip.data(), rows.data());
    return rc == ORBFE_OK || Fail("orbfe_fuse_batch_search", rc);
  }
  // the rows (first_target .. K-1, i in idx) again, with the points' records as they are now; idx ascending
  bool Repair(const std::vector<MapPointT*>& points, const std::vector<int32_t>& idx, int first_target) {
    std::vector<orbfe_kf_point> changed(idx.size());
    for (size_t j = 0; j < idx.size(); j++) {
      FillFusePoint(changed[j], points[(size_t)idx[j]]);
      rec[(size_t)idx[j]] = changed[j];
    }
    const int rc = orbfe_fuse_batch_search(batch, changed.data(), n, idx.data(), (int)idx.size(), first_target, nullptr, rows.data());
    return rc == ORBFE_OK || Fail("orbfe_fuse_batch_search (repair)", rc);
  }
};

// The map update of ORBmatcher::Fuse (L/src/ORBmatcher.cc:870-884) for one target from its rows, in point order on the live objects:
// the two tests of :787 are taken again (an earlier fusion can make a later point bad or put it into the keyframe).  A survivor whose
// GetDescriptor() bytes differ after a Replace is noted in `changed`.  Returns nFused.
template <class KeyFrameT, class MapPointT>
inline int FuseUpdate(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const orbfe_kf_result* rows, std::set<MapPointT*>& changed,
                      int th_low = 50) {
  int nFused = 0;
  for (size_t i = 0; i < vpMapPoints.size(); i++) {
    MapPointT* pMP = vpMapPoints[i];
    if (!pMP) continue;
    if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
    const int bestIdx = rows[i].best_idx;
    if (bestIdx < 0 || rows[i].best_dist > th_low) continue;
    MapPointT* pMPinKF = pKF->GetMapPoint((size_t)bestIdx);
    if (pMPinKF) {
      if (!pMPinKF->isBad()) {
        MapPointT* dying = pMPinKF->Observations() > pMP->Observations() ? pMP : pMPinKF;
        MapPointT* survivor = dying == pMP ? pMPinKF : pMP;
        uint8_t before[32];
        memcpy(before, survivor->GetDescriptor().ptr(0), 32);
        dying->Replace(survivor);
        if (memcmp(before, survivor->GetDescriptor().ptr(0), 32) != 0) changed.insert(survivor);
      }
    } else {
      pMP->AddObservation(pKF, (size_t)bestIdx);
      pKF->AddMapPoint(pMP, (size_t)bestIdx);
    }
    nFused++;
  }
  return nFused;
}

// Precondition: pCurrentKF->GetMapPointMatches() holds no point twice.  Returns the sum of the Fuse return values, or -1 after a
// failing library call was logged to stderr (no device, a keyframe beyond the library's limits):
// nothing is thrown, and the map is left as the calls made so far left it.
template <class KeyFrameT>
int SearchInNeighbors(KeyFrameT* pCurrentKF, bool bMonocular, float th = 3.0f) {
  typedef typename std::remove_pointer<decltype(pCurrentKF->GetMapPoint((size_t)0))>::type MapPointT;
  // Retrieve neighbor keyframes (:427-455)
  const int nn = bMonocular ? 20 : 10;
  const std::vector<KeyFrameT*> vpNeighKFs = pCurrentKF->GetBestCovisibilityKeyFrames(nn);
  std::vector<KeyFrameT*> vpTargetKFs;
  for (KeyFrameT* pKFi : vpNeighKFs) {
    if (pKFi->isBad() || pKFi->mnFuseTargetForKF == pCurrentKF->mnId) continue;
    vpTargetKFs.push_back(pKFi);
    pKFi->mnFuseTargetForKF = pCurrentKF->mnId;
    const std::vector<KeyFrameT*> vpSecondNeighKFs = pKFi->GetBestCovisibilityKeyFrames(5);   // extend to some second neighbors
    for (KeyFrameT* pKFi2 : vpSecondNeighKFs) {
      if (pKFi2->isBad() || pKFi2->mnFuseTargetForKF == pCurrentKF->mnId || pKFi2->mnId == pCurrentKF->mnId) continue;
      vpTargetKFs.push_back(pKFi2);
    }
  }
  int nFused = 0;
  // Search matches by projection from current KF in target KFs (:457-467)
  const std::vector<MapPointT*> vpMapPointMatches = pCurrentKF->GetMapPointMatches();
  if (!vpTargetKFs.empty() && !vpMapPointMatches.empty()) {
    FuseBatchRun<KeyFrameT, MapPointT> run;
    if (!run.Open(vpTargetKFs, vpMapPointMatches, th)) return -1;
    std::set<MapPointT*> changed;
    for (int k = 0; k < run.K; k++) {
      if (k > 0 && !changed.empty()) {
        std::vector<int32_t> idx;
        for (int i = 0; i < run.n; i++) {
          MapPointT* pMP = vpMapPointMatches[(size_t)i];
          if (pMP && !pMP->isBad() && changed.count(pMP)) idx.push_back(i);
        }
        changed.clear();
        if (!idx.empty() && !run.Repair(vpMapPointMatches, idx, k)) return -1;
      }
      nFused += FuseUpdate(vpTargetKFs[(size_t)k], vpMapPointMatches, run.rows.data() + (size_t)k * run.n, changed);
    }
  }
  // Search matches by projection from target KFs in current KF (:469-493): the candidates from the live map, each once
  std::vector<MapPointT*> vpFuseCandidates;
  for (KeyFrameT* pKFi : vpTargetKFs) {
    const std::vector<MapPointT*> vpMapPointsKFi = pKFi->GetMapPointMatches();
    for (MapPointT* pMP : vpMapPointsKFi) {
      if (!pMP) continue;
      if (pMP->isBad() || pMP->mnFuseCandidateForKF == pCurrentKF->mnId) continue;
      pMP->mnFuseCandidateForKF = pCurrentKF->mnId;
      vpFuseCandidates.push_back(pMP);
    }
  }
  if (!vpFuseCandidates.empty()) {
    FuseBatchRun<KeyFrameT, MapPointT> run;
    if (!run.Open(std::vector<KeyFrameT*>(1, pCurrentKF), vpFuseCandidates, th)) return -1;
    std::set<MapPointT*> changed;   // a survivor here is either done or inside the current keyframe: no repair
    nFused += FuseUpdate(pCurrentKF, vpFuseCandidates, run.rows.data(), changed);
  }
  // Update points (:495-505), one library call for all of them, and the connections in the covisibility graph (:508)
  if (RefreshMapPoints(pCurrentKF->GetMapPointMatches()) < 0) return -1;
  pCurrentKF->UpdateConnections();
  return nFused;
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
