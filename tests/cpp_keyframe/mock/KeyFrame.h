// KeyFrame.h -- MOCK (test infrastructure) of the reference's KeyFrame as far as NeedNewKeyFrame and the creation of close stereo points
// read and write it (Source/Libraries/ORB_SLAM2/include/KeyFrame.h): same member names, everything public.
#ifndef KEYFRAME_MOCK_KEYFRAME_H
#define KEYFRAME_MOCK_KEYFRAME_H
#include <mutex>
#include <vector>

#include "MapPoint.h"

namespace ORB_SLAM2 {
class KeyFrame {
 public:
  long unsigned int mnId = 0, mnFrameId = 0;
  int N = 0;
  std::vector<float> mvuRight;
  std::vector<MapPoint*> mvpMapPoints;
  std::mutex mMutexFeatures;

  std::vector<MapPoint*> GetMapPointMatches() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mvpMapPoints; }
  void AddMapPoint(MapPoint* pMP, const size_t& idx) {   // L/src/KeyFrame.cc:196-199
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    mvpMapPoints[idx] = pMP;
    LogCall(LOG_KF_ADD_MAP_POINT, (long)pMP->mnId, (long)idx);
  }
  int TrackedMapPoints(const int& minObs) {   // L/src/KeyFrame.cc:237-256
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    int nPoints = 0;
    const bool bCheckObs = minObs > 0;
    for (int i = 0; i < N; i++) {
      MapPoint* pMP = mvpMapPoints[i];
      if (pMP) {
        if (!pMP->isBad()) {
          if (bCheckObs) {
            if (mvpMapPoints[i]->Observations() >= minObs) nPoints++;
          } else
            nPoints++;
        }
      }
    }
    return nPoints;
  }
};

inline MapPoint::MapPoint(const Mat& Pos, KeyFrame* pRefKF, Map* pMap)
    : mnFirstKFid((long)pRefKF->mnId), mnFirstFrame((long)pRefKF->mnFrameId), mWorldPos(Pos), mpRefKF(pRefKF), mpMap(pMap) {
  mnId = NextId()++;
  LogCall(LOG_NEW_KF_POINT, (long)mnId, (long)pRefKF->mnId);
}
inline void MapPoint::AddObservation(KeyFrame* pKF, size_t idx) {
  std::unique_lock<std::mutex> lock(mMutexFeatures);
  if (mObservations.count(pKF)) return;
  mObservations[pKF] = idx;
  if (pKF->mvuRight[idx] >= 0) nObs += 2; else nObs++;
  LogCall(LOG_ADD_OBSERVATION, (long)mnId, (long)idx);
}
}  // namespace ORB_SLAM2
#endif
