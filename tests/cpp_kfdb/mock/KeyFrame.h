// KeyFrame.h -- MOCK (test infrastructure) of the reference's KeyFrame and Frame, as far as KeyFrameDatabase reads them
// (Source/Libraries/ORB_SLAM2/include/KeyFrame.h, Frame.h): same member names, the covisibility graph reduced to two stored lists.
#ifndef KFDB_MOCK_KEYFRAME_H
#define KFDB_MOCK_KEYFRAME_H
#include <map>
#include <set>
#include <vector>

namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
class BowVector : public std::map<WordId, WordValue> {};
}  // namespace DBoW2

namespace ORB_SLAM2 {
class KeyFrame {
 public:
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    return (int)mvpOrderedConnectedKeyFrames.size() < N ? mvpOrderedConnectedKeyFrames
                                                        : std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
  }
  std::set<KeyFrame*> GetConnectedKeyFrames() { return mspConnected; }
  bool isBad() { return mbBad; }
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  std::set<KeyFrame*> mspConnected;
  bool mbBad = false;
};

class Frame {
 public:
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
};
}  // namespace ORB_SLAM2
#endif
