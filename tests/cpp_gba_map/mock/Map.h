// Map.h -- MOCK (test infrastructure) of the reference's Map as far as the map update of LoopClosing::RunGlobalBundleAdjustment reads
// it (Source/Libraries/ORB_SLAM2/include/Map.h).
#ifndef GBA_MAP_MOCK_MAP_H
#define GBA_MAP_MOCK_MAP_H
#include <vector>

#include "KeyFrame.h"

namespace ORB_SLAM2 {
class Map {
 public:
  std::vector<MapPoint*> GetAllMapPoints() { return points; }
  std::vector<KeyFrame*> mvpKeyFrameOrigins;
  std::vector<MapPoint*> points;
};
}  // namespace ORB_SLAM2
#endif
