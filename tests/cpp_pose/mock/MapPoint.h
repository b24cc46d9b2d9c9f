// MapPoint.h -- MOCK (test infrastructure) of the reference's MapPoint, as far as Optimizer::PoseOptimization reads it
// (Source/Libraries/ORB_SLAM2/include/MapPoint.h): GetWorldPos() and the static mutex the optimiser holds while it reads positions.
#ifndef POSE_MOCK_MAPPOINT_H
#define POSE_MOCK_MAPPOINT_H
#include <mutex>

#include "../../../refactored_orb_slam2_amd/csrc/host/cvlite.h"

namespace ORB_SLAM2 {
class MapPoint {
 public:
  MapPoint(float x, float y, float z) : mWorldPos(3, 1, CV_32F) {
    mWorldPos.at<float>(0) = x;
    mWorldPos.at<float>(1) = y;
    mWorldPos.at<float>(2) = z;
  }
  cv::Mat GetWorldPos() { return mWorldPos.clone(); }
  inline static std::mutex mGlobalMutex;

 protected:
  cv::Mat mWorldPos;
};
}  // namespace ORB_SLAM2
#endif
