// test_pose_dropin.cpp -- orbfe_host::PoseOptimization (csrc/host/Optimizer_hip.h) on the mock Frame / MapPoint of this directory.
//   test_pose_dropin <in.bin> <out.bin>
// in.bin  (written by tests/test_pose_dropin_cpp.py): int32 n, n keypoints (28 bytes), n floats mvuRight, n int32 assigned,
//         int32 n_points, n_points x 3 floats, orbfe_pose_camera (88 bytes), 12 floats Tcw, n bytes mvbOutlier on entry
// out.bin: int32 return value, int32 SetPose calls, 12 floats (the first three rows of mTcw afterwards), n bytes mvbOutlier
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "mock/Frame.h"
#include "mock/MapPoint.h"
#include "../../refactored_orb_slam2_amd/csrc/host/Optimizer_hip.h"

using namespace ORB_SLAM2;

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0, np = 0;
  rd(f, &n, 1);
  Frame F;
  F.N = n;
  F.mvKeysUn.resize(n);
  F.mvuRight.resize(n);
  std::vector<int32_t> assigned(n);
  rd(f, F.mvKeysUn.data(), n);
  rd(f, F.mvuRight.data(), n);
  rd(f, assigned.data(), n);
  rd(f, &np, 1);
  std::vector<float> pts(3 * (size_t)np);
  rd(f, pts.data(), pts.size());
  orbfe_pose_camera cam;
  rd(f, &cam, 1);
  float T[12];
  rd(f, T, 12);
  std::vector<uint8_t> out0(n);
  rd(f, out0.data(), n);
  fclose(f);
  std::vector<std::unique_ptr<MapPoint>> owned;
  for (int i = 0; i < np; i++) owned.emplace_back(new MapPoint(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
  F.mvpMapPoints.assign(n, nullptr);
  F.mvbOutlier.resize(n);
  for (int i = 0; i < n; i++) {
    if (assigned[i] >= 0) F.mvpMapPoints[i] = owned[assigned[i]].get();
    F.mvbOutlier[i] = out0[i] != 0;
  }
  Frame::fx = cam.fx; Frame::fy = cam.fy; Frame::cx = cam.cx; Frame::cy = cam.cy;
  F.mbf = cam.mbf;
  F.mvInvLevelSigma2.assign(cam.inv_level_sigma2, cam.inv_level_sigma2 + cam.n_levels);
  F.mTcw = cv::Mat::eye(4, 4, CV_32F);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) F.mTcw.at<float>(r, c) = T[4 * r + c];
  const int32_t ret = orbfe_host::PoseOptimization(&F);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t calls = F.n_set_pose;
  fwrite(&ret, 4, 1, o);
  fwrite(&calls, 4, 1, o);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) fwrite(&F.mTcw.at<float>(r, c), 4, 1, o);
  for (int i = 0; i < n; i++) {
    const uint8_t b = F.mvbOutlier[i] ? 1 : 0;
    fwrite(&b, 1, 1, o);
  }
  fclose(o);
  printf("pose dropin ok: %d inliers\n", ret);
  return 0;
}
