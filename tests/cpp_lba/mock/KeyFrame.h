// KeyFrame.h -- MOCK (test infrastructure) of the reference's KeyFrame as far as Optimizer::LocalBundleAdjustment reads and writes it
// (Source/Libraries/ORB_SLAM2/include/KeyFrame.h): same member names; every write is counted or logged.
#ifndef LBA_MOCK_KEYFRAME_H
#define LBA_MOCK_KEYFRAME_H
#include <vector>

#include "MapPoint.h"

namespace ORB_SLAM2 {
class KeyFrame {
 public:
  bool isBad() { return bad; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return covisible; }
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  cv::Mat GetPose() { return Tcw.clone(); }
  void SetPose(const cv::Mat& T) {
    Tcw = T.clone();
    set_pose_calls++;
  }
  void EraseMapPointMatch(MapPoint* pMP) {
    for (size_t i = 0; i < mvpMapPoints.size(); i++)
      if (mvpMapPoints[i] == pMP) mvpMapPoints[i] = nullptr;
    erased.push_back(pMP);
  }
  long unsigned int mnId = 0;
  long unsigned int mnBALocalForKF = 0, mnBAFixedForKF = 0;
  bool bad = false;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  std::vector<float> mvInvLevelSigma2;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> covisible;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  cv::Mat Tcw;   // 4 x 4 float
  int set_pose_calls = 0;
  std::vector<MapPoint*> erased;
};
}  // namespace ORB_SLAM2
#endif
