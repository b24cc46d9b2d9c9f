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

#include <vector>

#include "../../../include/orbfe.h"
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

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
