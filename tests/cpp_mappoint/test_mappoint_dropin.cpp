// test_mappoint_dropin.cpp -- builds a scripted map on the mock MapPoint / KeyFrame, refreshes every point through
// csrc/host/MapPoint_hip.h and writes what the points hold afterwards, for tests/test_mappoint_dropin_cpp.py.
//   usage: test_mappoint_dropin script out mode      mode 0: RefreshMapPoints; 1: ComputeDistinctiveDescriptors, then UpdateNormalAndDepth
//   script (little endian): int32 n_levels, float scale_factors[n_levels], int32 n_kf, n_points;
//     per keyframe  int32 bad, float Ow[3], int32 n_keys, uint8 desc[n_keys][32], int32 octave[n_keys]
//     per point     int32 bad, float pos[3], int32 ref_kf, int32 n_obs, {int32 kf, int32 idx}[n_obs]
//   The keyframes live in one array, so the pointer order of a point's std::map is the order of the keyframe indices.
//   Before the calls every point holds the descriptor 0xEE.., the normal (7, 7, 7) and the distances -1 / -2.
//   output: per point uint8 desc[32], float normal[3], float min_distance, float max_distance.
//   Exit code 3 when a call reported a failure (no device): every point is then as it was.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "mock/MapPoint.h"
#include "../../refactored_orb_slam2_amd/csrc/host/MapPoint_hip.h"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

template <class T>
static bool rd(FILE* f, T* v, size_t n = 1) { return n == 0 || fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  const int mode = atoi(argv[3]);
  if (!in || !out) return 2;
  int32_t n_levels, n_kf, n_points;
  if (!rd(in, &n_levels) || n_levels < 1 || n_levels > 64) return 2;
  std::vector<float> sf((size_t)n_levels);
  if (!rd(in, sf.data(), sf.size()) || !rd(in, &n_kf) || !rd(in, &n_points) || n_kf < 0 || n_points < 0) return 2;
  std::vector<KeyFrame> kfs((size_t)n_kf);
  for (int k = 0; k < n_kf; k++) {
    KeyFrame& K = kfs[k];
    int32_t bad, n_keys;
    float Ow[3];
    if (!rd(in, &bad) || !rd(in, Ow, 3) || !rd(in, &n_keys) || n_keys < 0) return 2;
    K.mnId = (long unsigned int)k;
    K.bad = bad != 0;
    K.Ow = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) K.Ow.at<float>(r) = Ow[r];
    K.mDescriptors = cv::Mat(n_keys > 0 ? n_keys : 1, 32, CV_8U);
    if (!rd(in, K.mDescriptors.data, (size_t)n_keys * 32)) return 2;
    K.mDescriptors.rows = n_keys;
    std::vector<int32_t> oct((size_t)n_keys);
    if (!rd(in, oct.data(), oct.size())) return 2;
    K.mvKeysUn.resize((size_t)n_keys);
    for (int i = 0; i < n_keys; i++) K.mvKeysUn[i].octave = oct[i];
    K.mvScaleFactors = sf;
    K.mnScaleLevels = n_levels;
  }
  std::vector<std::unique_ptr<MapPoint>> pts;
  std::vector<MapPoint*> vpMPs;
  for (int p = 0; p < n_points; p++) {
    std::unique_ptr<MapPoint> M(new MapPoint);
    int32_t bad, ref_kf, n_obs;
    float pos[3];
    if (!rd(in, &bad) || !rd(in, pos, 3) || !rd(in, &ref_kf) || !rd(in, &n_obs) || n_obs < 0) return 2;
    M->bad = bad != 0;
    M->mWorldPos = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) M->mWorldPos.at<float>(r) = pos[r];
    M->mpRefKF = ref_kf >= 0 && ref_kf < n_kf ? &kfs[ref_kf] : nullptr;
    for (int j = 0; j < n_obs; j++) {
      int32_t o[2];
      if (!rd(in, o, 2) || o[0] < 0 || o[0] >= n_kf) return 2;
      M->mObservations[&kfs[o[0]]] = (size_t)o[1];
    }
    M->mDescriptor = cv::Mat(1, 32, CV_8U);
    memset(M->mDescriptor.data, 0xEE, 32);
    M->mNormalVector = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) M->mNormalVector.at<float>(r) = 7.0f;
    M->mfMinDistance = -1.0f;
    M->mfMaxDistance = -2.0f;
    vpMPs.push_back(M.get());
    if (p % 5 == 4) vpMPs.push_back(nullptr);   // the reference's vectors hold null entries
    pts.push_back(std::move(M));
  }
  bool failed = false;
  if (mode == 0) {
    failed = ORB_SLAM2::orbfe_host::RefreshMapPoints(vpMPs) < 0;
  } else {
    failed = ORB_SLAM2::orbfe_host::ComputeDistinctiveDescriptors(vpMPs) < 0;
    failed = ORB_SLAM2::orbfe_host::UpdateNormalAndDepth(vpMPs) < 0 || failed;
  }
  for (const std::unique_ptr<MapPoint>& M : pts) {
    fwrite(M->mDescriptor.data, 1, 32, out);
    float f[5] = {M->mNormalVector.at<float>(0), M->mNormalVector.at<float>(1), M->mNormalVector.at<float>(2), M->mfMinDistance,
                  M->mfMaxDistance};
    fwrite(f, 4, 5, out);
  }
  fclose(out);
  fclose(in);
  return failed ? 3 : 0;
}
