// MapPoint.h -- MOCK (test infrastructure) of the reference's MapPoint as far as Optimizer::LocalBundleAdjustment reads and writes it
// (Source/Libraries/ORB_SLAM2/include/MapPoint.h): same member names; every write is counted or logged so that a test can tell
// what the adapter did.
#ifndef LBA_MOCK_MAPPOINT_H
#define LBA_MOCK_MAPPOINT_H
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
  cv::Mat GetWorldPos() { return pos.clone(); }
  void SetWorldPos(const cv::Mat& X) {
    pos = X.clone();
    set_pos_calls++;
  }
  void UpdateNormalAndDepth() { update_calls++; }
  void EraseObservation(KeyFrame* pKF) {
    observations.erase(pKF);
    erased.push_back(pKF);
  }
  long unsigned int mnId = 0;
  long unsigned int mnBALocalForKF = 0;
  bool bad = false;
  std::map<KeyFrame*, size_t> observations;
  cv::Mat pos;   // 3 x 1 float
  int set_pos_calls = 0, update_calls = 0;
  std::vector<KeyFrame*> erased;
};
}  // namespace ORB_SLAM2
#endif
