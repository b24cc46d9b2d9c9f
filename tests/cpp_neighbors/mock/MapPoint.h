// MapPoint.h -- MOCK (test infrastructure) of the reference's MapPoint for tests/cpp_neighbors, with the map bookkeeping of
// Source/Libraries/ORB_SLAM2/src/MapPoint.cc read literally: AddObservation (:100-111), Replace (:172-206) and a
// ComputeDistinctiveDescriptors (:229-320) that really recomputes -- the descriptor with the least median distance to the others, in
// observation (keyframe pointer) order, the first on a tie.  No Map; everything public.
#ifndef MAPPOINT_H
#define MAPPOINT_H
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"

namespace ORB_SLAM2 {

class MapPoint {
 public:
  MapPoint(const cv::Mat& Pos, const cv::Mat& Normal, const cv::Mat& Desc, float minD, float maxD)
      : mWorldPos(Pos.clone()), mNormalVector(Normal.clone()), mDescriptor(Desc.clone()), mfMinDistance(minD), mfMaxDistance(maxD) {}
  cv::Mat GetWorldPos() { return mWorldPos.clone(); }
  cv::Mat GetNormal() { return mNormalVector.clone(); }
  KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
  std::map<KeyFrame*, std::size_t> GetObservations() { return mObservations; }
  int Observations() { return nObs; }
  void AddObservation(KeyFrame* pKF, std::size_t idx) {
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2;
    else nObs++;
  }
  int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
  bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
  void SetBadFlag() { mbBad = true; }
  bool isBad() { return mbBad; }
  void Replace(MapPoint* pMP) {
    if (pMP->mnId == this->mnId) return;
    std::map<KeyFrame*, std::size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    const int nvisible = mnVisible, nfound = mnFound;
    mpReplaced = pMP;
    for (auto& kv : obs) {
      KeyFrame* pKF = kv.first;
      if (!pMP->IsInKeyFrame(pKF)) {
        pKF->ReplaceMapPointMatch(kv.second, pMP);
        pMP->AddObservation(pKF, kv.second);
      } else {
        pKF->EraseMapPointMatch(kv.second);
      }
    }
    pMP->IncreaseFound(nfound);
    pMP->IncreaseVisible(nvisible);
    pMP->ComputeDistinctiveDescriptors();
  }
  MapPoint* GetReplaced() { return mpReplaced; }
  void IncreaseVisible(int n = 1) { mnVisible += n; }
  void IncreaseFound(int n = 1) { mnFound += n; }
  static int Distance(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
  }
  void ComputeDistinctiveDescriptors() {
    nDescriptorUpdates++;
    if (mbBad || mObservations.empty()) return;
    std::vector<const uint8_t*> v;
    for (auto& kv : mObservations)
      if (!kv.first->isBad()) v.push_back(kv.first->mDescriptors.ptr((int)kv.second));
    if (v.empty()) return;
    const size_t N = v.size();
    int BestMedian = INT_MAX, BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
      std::vector<int> vDists(N);
      for (size_t j = 0; j < N; j++) vDists[j] = Distance(v[i], v[j]);
      std::sort(vDists.begin(), vDists.end());
      const int median = vDists[(size_t)(0.5 * (N - 1))];
      if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    cv::Mat d(1, 32, CV_8U);
    memcpy(d.ptr(0), v[(size_t)BestIdx], 32);
    mDescriptor = d;
  }
  cv::Mat GetDescriptor() { return mDescriptor.clone(); }
  float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
  float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
  int PredictScale(const float& currentDist, KeyFrame* pKF) { return Predict(currentDist, pKF->mfLogScaleFactor, pKF->mnScaleLevels); }
  int PredictScale(const float& currentDist, Frame* pF) { return Predict(currentDist, pF->mfLogScaleFactor, pF->mnScaleLevels); }
  int Predict(float d, float logsf, int nl) {
    const float ratio = mfMaxDistance / d;
    int nScale = (int)ceil(log(ratio) / logsf);
    if (nScale < 0) nScale = 0;
    else if (nScale >= nl) nScale = nl - 1;
    return nScale;
  }

 public:
  long unsigned int mnId = 0;
  long unsigned int mnFuseCandidateForKF = 0;
  int nObs = 0;
  float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0;
  bool mbTrackInView = false;
  int mnTrackScaleLevel = 0;
  float mTrackViewCos = 0;
  long unsigned int mnLastFrameSeen = 0;
  int nDescriptorUpdates = 0;   // mock only
  cv::Mat mWorldPos;
  std::map<KeyFrame*, std::size_t> mObservations;
  cv::Mat mNormalVector;
  cv::Mat mDescriptor;
  KeyFrame* mpRefKF = nullptr;
  int mnVisible = 1, mnFound = 1;
  bool mbBad = false;
  MapPoint* mpReplaced = nullptr;
  float mfMinDistance;
  float mfMaxDistance;
  std::mutex mMutexFeatures, mMutexPos;
};

inline std::set<MapPoint*> KeyFrame::GetMapPoints() {   // KeyFrame.cc:237-250: every match that exists and is not bad
  std::set<MapPoint*> s;
  for (MapPoint* pMP : mvpMapPoints)
    if (pMP && !pMP->isBad()) s.insert(pMP);
  return s;
}

}  // namespace ORB_SLAM2
#endif
