// MapPoint.h -- MOCK (test infrastructure) of the reference's MapPoint as far as Optimizer::BundleAdjustment and
// Tracking::CreateInitialMapMonocular read and write it (Source/Libraries/ORB_SLAM2/include/MapPoint.h): same member names; every
// write is counted so that a test can tell what the adapter did.
#ifndef BA_MOCK_MAPPOINT_H
#define BA_MOCK_MAPPOINT_H
#include <stddef.h>

#include <map>
#include <vector>

#include "../../../refactored_orb_slam2_amd/csrc/host/cvlite.h"

namespace ORB_SLAM2 {
class KeyFrame;

class MapPoint {
 public:
  bool isBad() { return bad; }
  std::map<KeyFrame*, size_t> GetObservations() { return observations; }
  int GetIndexInKeyFrame(KeyFrame* pKF) {
    const auto it = observations.find(pKF);
    return it == observations.end() ? -1 : (int)it->second;
  }
  cv::Mat GetWorldPos() { return pos.clone(); }
  void SetWorldPos(const cv::Mat& X) {
    pos = X.clone();
    set_pos_calls++;
  }
  void UpdateNormalAndDepth() { update_calls++; }
  long unsigned int mnId = 0;
  long unsigned int mnBAGlobalForKF = 0;
  bool bad = false;
  std::map<KeyFrame*, size_t> observations;
  cv::Mat pos;       // 3 x 1 float
  cv::Mat mPosGBA;   // empty until a loop's adjustment writes it
  int set_pos_calls = 0, update_calls = 0;
};
}  // namespace ORB_SLAM2
#endif
