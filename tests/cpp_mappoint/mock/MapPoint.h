// MapPoint.h -- MOCK (test infrastructure) of the reference's MapPoint as far as the batched ComputeDistinctiveDescriptors /
// UpdateNormalAndDepth of csrc/host/MapPoint_hip.h read and write it (Source/Libraries/ORB_SLAM2/include/MapPoint.h): same member
// names, everything public.
#ifndef MAPPOINT_MOCK_MAPPOINT_H
#define MAPPOINT_MOCK_MAPPOINT_H
#include <stddef.h>

#include <map>
#include <mutex>

#include "KeyFrame.h"

namespace ORB_SLAM2 {
class MapPoint {
 public:
  bool isBad() { return bad; }
  std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
  KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
  cv::Mat GetWorldPos() { return mWorldPos.clone(); }
  bool bad = false;
  std::map<KeyFrame*, size_t> mObservations;
  KeyFrame* mpRefKF = nullptr;
  cv::Mat mWorldPos;       // 3 x 1 float
  cv::Mat mDescriptor;     // 1 x 32 bytes
  cv::Mat mNormalVector;   // 3 x 1 float
  float mfMinDistance = 0, mfMaxDistance = 0;
  std::mutex mMutexFeatures, mMutexPos;
};
}  // namespace ORB_SLAM2
#endif
