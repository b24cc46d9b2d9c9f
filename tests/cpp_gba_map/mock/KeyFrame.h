// KeyFrame.h -- MOCK (test infrastructure) of the reference's KeyFrame as far as the map update of
// LoopClosing::RunGlobalBundleAdjustment reads and writes it (Source/Libraries/ORB_SLAM2/include/KeyFrame.h): same member names; every
// write through a method is counted.  SetPose keeps the inverse with plain double arithmetic -- the adapter does not read it.
#ifndef GBA_MAP_MOCK_KEYFRAME_H
#define GBA_MAP_MOCK_KEYFRAME_H
#include <set>

#include "MapPoint.h"

namespace ORB_SLAM2 {
class KeyFrame {
 public:
  std::set<KeyFrame*> GetChilds() { return mspChildrens; }
  cv::Mat GetPose() { return Tcw.clone(); }
  cv::Mat GetPoseInverse() { return Twc.clone(); }
  void SetPose(const cv::Mat& T) {
    Tcw = T.clone();
    Twc = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
      double o = 0;
      for (int c = 0; c < 3; c++) {
        Twc.at<float>(r, c) = T.at<float>(c, r);
        o -= (double)T.at<float>(c, r) * (double)T.at<float>(c, 3);
      }
      Twc.at<float>(r, 3) = (float)o;
    }
    set_pose_calls++;
  }
  long unsigned int mnId = 0;
  long unsigned int mnBAGlobalForKF = 0;
  float mb = 0;
  std::set<KeyFrame*> mspChildrens;
  cv::Mat Tcw, Twc;    // 4 x 4 float
  cv::Mat mTcwGBA;     // empty unless the adjustment wrote it
  cv::Mat mTcwBefGBA;  // empty until the map update writes it
  int set_pose_calls = 0;
};
}  // namespace ORB_SLAM2
#endif
