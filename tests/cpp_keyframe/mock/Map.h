// Map.h -- MOCK (test infrastructure) of the reference's Map as far as the keyframe decision and the creation of close stereo points use
// it (Source/Libraries/ORB_SLAM2/include/Map.h).
#ifndef KEYFRAME_MOCK_MAP_H
#define KEYFRAME_MOCK_MAP_H
#include <vector>

#include "MapPoint.h"

namespace ORB_SLAM2 {
class Map {
 public:
  long unsigned int mnKeyFrames = 0;
  std::vector<MapPoint*> mvpAdded;   // the mock keeps the order of AddMapPoint (the reference holds a std::set)
  long unsigned int KeyFramesInMap() { return mnKeyFrames; }
  void AddMapPoint(MapPoint* pMP) {
    mvpAdded.push_back(pMP);
    LogCall(LOG_MAP_ADD, (long)pMP->mnId, 0);
  }
};
}  // namespace ORB_SLAM2
#endif
