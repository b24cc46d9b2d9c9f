// Frame.h -- MOCK (test infrastructure) of the reference's Frame as far as the keyframe decision and the creation of close stereo points
// read and write it (Source/Libraries/ORB_SLAM2/include/Frame.h): same member names.  UnprojectStereo is Frame.cc:668-679 in the
// arithmetic cv::Mat gives it.
#ifndef KEYFRAME_MOCK_FRAME_H
#define KEYFRAME_MOCK_FRAME_H
#include <stdint.h>

#include <vector>

#include "KeyFrame.h"

namespace ORB_SLAM2 {
struct Point2f { float x, y; };
struct KeyPoint {   // cv::KeyPoint: 28 bytes
  Point2f pt;
  float size, angle, response;
  int octave, class_id;
};
struct Descriptors {   // cv::Mat of N x 32 bytes
  std::vector<uint8_t> bytes;
  const uint8_t* ptr(int row) const { return bytes.data() + (size_t)row * 32; }
};

class Frame {
 public:
  static float cx, cy, invfx, invfy;
  long unsigned int mnId = 0;
  int N = 0;
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvDepth;
  Descriptors mDescriptors;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  std::vector<float> mvScaleFactors;
  Mat mRwc, mOw;

  Mat GetRotationInverse() { return mRwc; }
  Mat GetCameraCenter() { return mOw; }
  Mat UnprojectStereo(const int& i) {
    const float z = mvDepth[i];
    Mat out;
    if (z > 0) {
      const float u = mvKeysUn[i].pt.x, v = mvKeysUn[i].pt.y;
      const float x = (u - cx) * z * invfx, y = (v - cy) * z * invfy;
      for (int r = 0; r < 3; r++) {
        const float t = mRwc.v[3 * r] * x + mRwc.v[3 * r + 1] * y + mRwc.v[3 * r + 2] * z;
        out.v[r] = (float)((double)t * 1.0 + (double)mOw.v[r] * 1.0);
      }
    }
    return out;
  }
};
inline MapPoint::MapPoint(const Mat& Pos, Map* pMap, Frame* pFrame, const int& idxF)
    : mnFirstKFid(-1), mnFirstFrame((long)pFrame->mnId), mWorldPos(Pos), mpFromFrame(pFrame), mnFromIdx(idxF), mpMap(pMap) {
  mnId = NextId()++;
  LogCall(LOG_NEW_FRAME_POINT, (long)mnId, (long)idxF);
}
}  // namespace ORB_SLAM2
#endif
