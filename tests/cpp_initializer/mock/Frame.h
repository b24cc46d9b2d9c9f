// Frame.h -- MOCK (test infrastructure) of the reference's Frame, as far as Initializer reads it
// (Source/Libraries/ORB_SLAM2/include/Frame.h): same member names.
#ifndef INITIALIZER_MOCK_FRAME_H
#define INITIALIZER_MOCK_FRAME_H
#include <vector>

#include "../../../refactored_orb_slam2_amd/csrc/host/cvlite.h"

namespace ORB_SLAM2 {
class Frame {
 public:
  std::vector<cv::KeyPoint> mvKeysUn;
  cv::Mat mK;   // 3 x 3 float
};
}  // namespace ORB_SLAM2
#endif
