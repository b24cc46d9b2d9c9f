// Frame.h -- MOCK (test infrastructure) of the reference's Frame, as far as Optimizer::PoseOptimization reads and writes it
// (Source/Libraries/ORB_SLAM2/include/Frame.h): same member names and static-ness, plus SetPose.
#ifndef POSE_MOCK_FRAME_H
#define POSE_MOCK_FRAME_H
#include <vector>

#include "../../../refactored_orb_slam2_amd/csrc/host/cvlite.h"

namespace ORB_SLAM2 {
class MapPoint;

class Frame {
 public:
  void SetPose(cv::Mat Tcw) {
    mTcw = Tcw.clone();
    n_set_pose++;
  }
  inline static float fx = 0, fy = 0, cx = 0, cy = 0;
  float mbf = 0;
  int N = 0;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  std::vector<float> mvInvLevelSigma2;
  cv::Mat mTcw;
  int n_set_pose = 0;   // test bookkeeping
};
}  // namespace ORB_SLAM2
#endif
