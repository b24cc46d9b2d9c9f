// MapPoint.h -- MOCK (test infrastructure) of the reference's MapPoint as far as the local map of a tracked frame reads and writes it
// (Source/Libraries/ORB_SLAM2/include/MapPoint.h): same member names, everything public.
#ifndef LOCALMAP_MOCK_MAPPOINT_H
#define LOCALMAP_MOCK_MAPPOINT_H
#include <stddef.h>

#include <map>
#include <mutex>

#include "KeyFrame.h"

namespace ORB_SLAM2 {
class MapPoint {
 public:
  std::map<KeyFrame*, size_t> mObservations;
  int nObs = 0;
  bool mbBad = false;
  long unsigned int mnTrackReferenceForFrame = 0;
  long unsigned int mnLastFrameSeen = 0;
  std::mutex mMutexFeatures, mMutexPos;

  bool isBad() { std::unique_lock<std::mutex> lock(mMutexFeatures); std::unique_lock<std::mutex> lock2(mMutexPos); return mbBad; }
  std::map<KeyFrame*, size_t> GetObservations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mObservations; }
  int Observations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return nObs; }
};
}  // namespace ORB_SLAM2
#endif
