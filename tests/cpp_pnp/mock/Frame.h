// Frame.h -- MOCK (test infrastructure) of the reference's Frame and MapPoint, as far as PnPsolver reads them
// (Source/Libraries/ORB_SLAM2/include/Frame.h, MapPoint.h): same member names.
#ifndef PNP_MOCK_FRAME_H
#define PNP_MOCK_FRAME_H
#include <vector>

#include "../../../refactored_orb_slam2_amd/csrc/host/cvlite.h"

namespace ORB_SLAM2 {
class MapPoint {
 public:
  bool isBad() { return bad; }
  cv::Mat GetWorldPos() { return pos.clone(); }
  bool bad = false;
  cv::Mat pos;   // 3 x 1 float
};

class Frame {
 public:
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvLevelSigma2;
  std::vector<MapPoint*> mvpMapPoints;
  float fx = 0, fy = 0, cx = 0, cy = 0;
};
}  // namespace ORB_SLAM2
#endif
