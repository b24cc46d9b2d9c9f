// KeyFrame.h -- MOCK (test infrastructure) of the reference's KeyFrame as far as Optimizer::BundleAdjustment and
// Tracking::CreateInitialMapMonocular read and write it (Source/Libraries/ORB_SLAM2/include/KeyFrame.h): same member names; every
// write is counted.
#ifndef BA_MOCK_KEYFRAME_H
#define BA_MOCK_KEYFRAME_H
#include <vector>

#include "MapPoint.h"

namespace ORB_SLAM2 {
class KeyFrame {
 public:
  bool isBad() { return bad; }
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  cv::Mat GetPose() { return Tcw.clone(); }
  void SetPose(const cv::Mat& T) {
    Tcw = T.clone();
    set_pose_calls++;
  }
  long unsigned int mnId = 0;
  long unsigned int mnBAGlobalForKF = 0;
  bool bad = false;
  int N = 0;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  std::vector<float> mvInvLevelSigma2;
  std::vector<MapPoint*> mvpMapPoints;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  cv::Mat Tcw;       // 4 x 4 float
  cv::Mat mTcwGBA;   // empty until a loop's adjustment writes it
  int set_pose_calls = 0;
};
}  // namespace ORB_SLAM2
#endif
