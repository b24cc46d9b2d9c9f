// LocalMapping.h -- MOCK (test infrastructure) of the reference's LocalMapping as far as Tracking::NeedNewKeyFrame asks it
// (Source/Libraries/ORB_SLAM2/include/LocalMapping.h).
#ifndef KEYFRAME_MOCK_LOCALMAPPING_H
#define KEYFRAME_MOCK_LOCALMAPPING_H
#include "MapPoint.h"

namespace ORB_SLAM2 {
class LocalMapping {
 public:
  bool mbStopped = false, mbStopRequested = false, mbAcceptKeyFrames = true;
  int mnQueue = 0, mnInterrupts = 0;
  bool isStopped() { return mbStopped; }
  bool stopRequested() { return mbStopRequested; }
  bool AcceptKeyFrames() { return mbAcceptKeyFrames; }
  int KeyframesInQueue() { return mnQueue; }
  void InterruptBA() {
    mnInterrupts++;
    LogCall(LOG_INTERRUPT_BA, 0, 0);
  }
};
}  // namespace ORB_SLAM2
#endif
