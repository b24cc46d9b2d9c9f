// MapPoint.h -- MOCK (test infrastructure) of the reference's MapPoint as far as the keyframe decision and the creation of close stereo
// points read and write it (Source/Libraries/ORB_SLAM2/include/MapPoint.h): same member names, everything public.  Every call that
// the creation makes is appended to a log, so that two worlds can be compared call for call.
#ifndef KEYFRAME_MOCK_MAPPOINT_H
#define KEYFRAME_MOCK_MAPPOINT_H
#include <stddef.h>

#include <array>
#include <map>
#include <mutex>
#include <vector>

namespace ORB_SLAM2 {
class KeyFrame;
class Frame;
class Map;

// what stands for cv::Mat here: at<float>(r, c) / at<float>(r) over nine floats
struct Mat {
  float v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  template <class T> T at(int r, int c) const { return v[3 * r + c]; }
  template <class T> T at(int r) const { return v[r]; }
};

enum { LOG_NEW_KF_POINT = 1, LOG_NEW_FRAME_POINT, LOG_ADD_OBSERVATION, LOG_KF_ADD_MAP_POINT, LOG_DESCRIPTORS, LOG_NORMAL_DEPTH, LOG_MAP_ADD,
       LOG_INTERRUPT_BA };
inline std::vector<std::array<long, 3> >*& Log() {
  static std::vector<std::array<long, 3> >* log = nullptr;
  return log;
}
inline void LogCall(long what, long id, long arg) { if (Log()) Log()->push_back({what, id, arg}); }

class MapPoint {
 public:
  static long unsigned int& NextId() { static long unsigned int n = 0; return n; }
  long unsigned int mnId;
  long int mnFirstKFid, mnFirstFrame;
  int nObs = 0;
  bool mbBad = false;
  Mat mWorldPos;
  KeyFrame* mpRefKF = nullptr;
  Frame* mpFromFrame = nullptr;   // the mock's own: the frame of the second constructor
  int mnFromIdx = -1;
  Map* mpMap = nullptr;
  std::map<KeyFrame*, size_t> mObservations;
  std::mutex mMutexFeatures, mMutexPos;

  MapPoint() : mnId(NextId()++), mnFirstKFid(-2), mnFirstFrame(-2) {}   // a point the scene starts with
  MapPoint(const Mat& Pos, KeyFrame* pRefKF, Map* pMap);                   // L/src/MapPoint.cc:32-47
  MapPoint(const Mat& Pos, Map* pMap, Frame* pFrame, const int& idxF);     // L/src/MapPoint.cc:49-77
  bool isBad() { std::unique_lock<std::mutex> lock(mMutexFeatures); std::unique_lock<std::mutex> lock2(mMutexPos); return mbBad; }
  int Observations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return nObs; }
  void AddObservation(KeyFrame* pKF, size_t idx);                           // L/src/MapPoint.cc:100-111
  void ComputeDistinctiveDescriptors() { LogCall(LOG_DESCRIPTORS, (long)mnId, 0); }
  void UpdateNormalAndDepth() { LogCall(LOG_NORMAL_DEPTH, (long)mnId, 0); }
};
}  // namespace ORB_SLAM2
#endif
