// Map.h -- MOCK (test infrastructure) of the reference's Map as far as Optimizer::GlobalBundleAdjustemnt reads it
// (Source/Libraries/ORB_SLAM2/include/Map.h).
#ifndef BA_MOCK_MAP_H
#define BA_MOCK_MAP_H
#include <vector>

#include "KeyFrame.h"

namespace ORB_SLAM2 {
class Map {
 public:
  std::vector<KeyFrame*> GetAllKeyFrames() { return keyframes; }
  std::vector<MapPoint*> GetAllMapPoints() { return points; }
  std::vector<KeyFrame*> keyframes;
  std::vector<MapPoint*> points;
};
}  // namespace ORB_SLAM2
#endif
