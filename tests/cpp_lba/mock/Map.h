// Map.h -- MOCK (test infrastructure) of the reference's Map as far as Optimizer::LocalBundleAdjustment touches it: the mutex it
// holds while it writes the result back (Source/Libraries/ORB_SLAM2/include/Map.h).
#ifndef LBA_MOCK_MAP_H
#define LBA_MOCK_MAP_H
#include <mutex>

namespace ORB_SLAM2 {
class Map {
 public:
  std::mutex mMutexMapUpdate;
};
}  // namespace ORB_SLAM2
#endif
