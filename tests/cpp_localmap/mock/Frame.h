// Frame.h -- MOCK (test infrastructure) of the reference's Frame as far as Tracking::UpdateLocalMap and the first half of
// Tracking::SearchLocalPoints read and write it (Source/Libraries/ORB_SLAM2/include/Frame.h): same member names.
#ifndef LOCALMAP_MOCK_FRAME_H
#define LOCALMAP_MOCK_FRAME_H
#include <vector>

#include "MapPoint.h"

namespace ORB_SLAM2 {
class Frame {
 public:
  long unsigned int mnId = 0;
  int N = 0;
  std::vector<MapPoint*> mvpMapPoints;
};
}  // namespace ORB_SLAM2
#endif
