// KeyFrame.h -- MOCK (test infrastructure) of the reference's KeyFrame as far as Tracking::UpdateLocalKeyFrames and
// Tracking::UpdateLocalPoints read and write it (Source/Libraries/ORB_SLAM2/include/KeyFrame.h): same member names, everything public.
#ifndef LOCALMAP_MOCK_KEYFRAME_H
#define LOCALMAP_MOCK_KEYFRAME_H
#include <mutex>
#include <set>
#include <vector>

namespace ORB_SLAM2 {
class MapPoint;
class KeyFrame {
 public:
  long unsigned int mnId = 0;
  long unsigned int mnTrackReferenceForFrame = 0;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  KeyFrame* mpParent = nullptr;
  std::set<KeyFrame*> mspChildrens;
  bool mbBad = false;
  std::mutex mMutexConnections, mMutexFeatures;

  bool isBad() { std::unique_lock<std::mutex> lock(mMutexConnections); return mbBad; }
  std::vector<MapPoint*> GetMapPointMatches() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mvpMapPoints; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {   // KeyFrame.cc:180-187
    std::unique_lock<std::mutex> lock(mMutexConnections);
    if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
  }
  std::set<KeyFrame*> GetChilds() { std::unique_lock<std::mutex> lock(mMutexConnections); return mspChildrens; }
  KeyFrame* GetParent() { std::unique_lock<std::mutex> lock(mMutexConnections); return mpParent; }
};
}  // namespace ORB_SLAM2
#endif
