// MapPoint_hip.h -- host-side adapter: MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth for a whole vector
// of map points in ONE call of liborbfe (include/orbfe.h: orbfe_refresh_map_points).
//
// The reference refreshes a map point with these two member functions at the end of every step that creates, fuses or moves it
// (Source/Libraries/ORB_SLAM2/src/MapPoint.cc:229-320, :340-381; call sites in INTEGRATION.md), one point at a time on the host.
// The functions here take the points of such a step together, walk GetObservations() of each in map order -- the order the
// reference's own loops see --, ask the library for the chosen descriptor, the mean viewing direction and the distance range of all
// of them at once, and write mDescriptor / mNormalVector / mfMinDistance / mfMaxDistance under the locks the reference takes.
// Skipped, as in the reference: a null entry, a bad point, a point without observations; the descriptor of a point whose observing
// keyframes are all bad.  A point whose reference keyframe is not among its observations is left alone and logged (the reference
// would insert a zero index into its copy of the map and read keypoint 0).
//
// A template over the MapPoint type (the KeyFrame type is the key of its observation map) so that it compiles (and is unit-tested,
// tests/cpp_mappoint) without the reference tree.  A failing library call is logged to stderr, never thrown, and leaves every point
// as it was.  The four members written are protected in the reference: declare
//     template <class T> friend struct orbfe_host::MapPointRefresh;
// in class MapPoint.
//
// Members used (same names as the reference):
//   MapPoint: isBad(), GetObservations(), GetReferenceKeyFrame(), GetWorldPos(), mMutexFeatures, mMutexPos, mDescriptor,
//             mNormalVector, mfMinDistance, mfMaxDistance
//   KeyFrame: isBad(), GetCameraCenter(), mDescriptors (N x 32, CV_8U, continuous), mvKeysUn, mvScaleFactors, mnScaleLevels
#pragma once
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../../include/orbfe.h"

namespace ORB_SLAM2 {
namespace orbfe_host {

template <class MapPointT>
struct MapPointRefresh {
  typedef decltype(std::declval<MapPointT>().GetObservations()) ObservationsT;
  typedef typename std::remove_pointer<typename ObservationsT::key_type>::type KeyFrameT;

  // flags: ORBFE_MP_DESCRIPTOR, ORBFE_MP_NORMAL_DEPTH or both.  Returns the number of points refreshed, -1 when the library call failed.
  static int Run(const std::vector<MapPointT*>& vpMPs, int flags) {
    std::vector<MapPointT*> vpTaken;
    std::vector<orbfe_mp_point> points;
    std::vector<orbfe_mp_obs> obs;
    std::vector<orbfe_mp_keyframe> table;
    std::vector<float> positions;
    std::map<KeyFrameT*, int32_t> row;
    std::vector<float> scale_factors;
    for (MapPointT* pMP : vpMPs) {
      if (!pMP || pMP->isBad()) continue;   // :238, :348
      const ObservationsT observations = pMP->GetObservations();
      if (observations.empty()) continue;   // :242, :355
      KeyFrameT* pRefKF = pMP->GetReferenceKeyFrame();
      const cv::Mat Pos = pMP->GetWorldPos();
      orbfe_mp_point Q;
      Q.obs_offset = (int32_t)obs.size();
      Q.n_obs = (int32_t)observations.size();
      Q.ref = -1;
      Q.ref_octave = 0;
      int32_t j = 0;
      for (typename ObservationsT::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; ++mit, ++j) {
        KeyFrameT* pKF = mit->first;
        typename std::map<KeyFrameT*, int32_t>::iterator it = row.find(pKF);
        if (it == row.end()) {
          orbfe_mp_keyframe K;
          memset(&K, 0, sizeof(K));
          const bool usable = pKF->mDescriptors.cols == 32 && pKF->mDescriptors.isContinuous();
          K.desc = usable ? (uint64_t)(uintptr_t)pKF->mDescriptors.data : 0;
          K.n_keys = usable ? pKF->mDescriptors.rows : 0;
          K.bad = pKF->isBad() ? 1 : 0;
          const cv::Mat Ow = pKF->GetCameraCenter();
          for (int r = 0; r < 3; r++) K.Ow[r] = Ow.template at<float>(r);
          it = row.insert(std::make_pair(pKF, (int32_t)table.size())).first;
          table.push_back(K);
        }
        orbfe_mp_obs o;
        o.kf = it->second;
        o.idx = (int32_t)mit->second;
        obs.push_back(o);
        if (pKF == pRefKF) {
          Q.ref = j;
          Q.ref_octave = pKF->mvKeysUn[mit->second].octave;   // :372
        }
      }
      if (Q.ref < 0) {
        fprintf(stderr, "orbfe_host::MapPointRefresh: a point's reference keyframe is not among its observations; the point is left alone\n");
        obs.resize((size_t)Q.obs_offset);
        continue;
      }
      if (scale_factors.empty()) scale_factors.assign(pRefKF->mvScaleFactors.begin(), pRefKF->mvScaleFactors.begin() + pRefKF->mnScaleLevels);
      for (int r = 0; r < 3; r++) positions.push_back(Pos.template at<float>(r));
      points.push_back(Q);
      vpTaken.push_back(pMP);
    }
    if (points.empty()) return 0;
    std::vector<orbfe_mp_update> updates(points.size());
    const int rc = orbfe_refresh_map_points(table.data(), (int)table.size(), obs.data(), (int)obs.size(), points.data(), positions.data(),
                                            (int)points.size(), scale_factors.data(), (int)scale_factors.size(), flags, updates.data());
    if (rc != ORBFE_OK) {
      fprintf(stderr, "orbfe_host::MapPointRefresh: orbfe_refresh_map_points failed: %s (code %d)\n", orbfe_last_error(), rc);
      return -1;
    }
    int n = 0;
    for (size_t p = 0; p < points.size(); p++) {
      const orbfe_mp_update& U = updates[p];
      MapPointT* pMP = vpTaken[p];
      if (U.status != ORBFE_MP_UPDATED) {
        fprintf(stderr, "orbfe_host::MapPointRefresh: a point was refused (an observation outside its keyframe); it is left alone\n");
        continue;
      }
      if ((flags & ORBFE_MP_DESCRIPTOR) && U.best >= 0) {   // :257: no live descriptor, no change
        cv::Mat d(1, 32, CV_8U);
        memcpy(d.data, U.desc, 32);
        std::unique_lock<std::mutex> lock(pMP->mMutexFeatures);
        pMP->mDescriptor = d;
      }
      if (flags & ORBFE_MP_NORMAL_DEPTH) {
        cv::Mat normal(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) normal.template at<float>(r) = U.normal[r];
        std::unique_lock<std::mutex> lock3(pMP->mMutexPos);
        pMP->mfMaxDistance = U.max_distance;
        pMP->mfMinDistance = U.min_distance;
        pMP->mNormalVector = normal;
      }
      n++;
    }
    return n;
  }
};

// pMP->ComputeDistinctiveDescriptors() for every point of the vector
template <class MapPointT>
int ComputeDistinctiveDescriptors(const std::vector<MapPointT*>& vpMPs) {
  return MapPointRefresh<MapPointT>::Run(vpMPs, ORBFE_MP_DESCRIPTOR);
}
// pMP->UpdateNormalAndDepth() for every point of the vector
template <class MapPointT>
int UpdateNormalAndDepth(const std::vector<MapPointT*>& vpMPs) {
  return MapPointRefresh<MapPointT>::Run(vpMPs, ORBFE_MP_NORMAL_DEPTH);
}
// both, as the reference's call sites pair them, in one library call
template <class MapPointT>
int RefreshMapPoints(const std::vector<MapPointT*>& vpMPs) {
  return MapPointRefresh<MapPointT>::Run(vpMPs, ORBFE_MP_DESCRIPTOR | ORBFE_MP_NORMAL_DEPTH);
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
