// test_gba_map_dropin.cpp -- orbfe_host::RunGlobalBundleAdjustmentUpdateMap (csrc/host/LoopClosing_hip.h) on the mock Map / KeyFrame /
// MapPoint of this directory:
//   test_gba_map_dropin <in.bin> <out.bin>
// in.bin  (written by tests/test_gba_map_dropin_cpp.py): int32 nLoopKF, float mb; int32 NK, NK keyframes (int32 parent index or -1 for
//         an origin, int32 optimised, 12 floats of Tcw, 12 floats of mTcwGBA -- read only when optimised); int32 NM, NM map points
//         (int32 bad, int32 optimised, int32 reference keyframe index, 3 floats, 3 floats of mPosGBA -- read only when optimised)
// out.bin int32 return value; NK x (int32 SetPose calls, 12 floats of Tcw, int32 mnBAGlobalForKF, int32 mTcwGBA rows, 12 floats of it
//         or zeros, int32 mTcwBefGBA rows, 12 floats of it or zeros); NM x (int32 SetWorldPos calls, int32 UpdateNormalAndDepth
//         calls, 3 floats)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "mock/KeyFrame.h"
#include "mock/Map.h"
#include "../../refactored_orb_slam2_amd/csrc/host/LoopClosing_hip.h"

using namespace ORB_SLAM2;

static void wr32(FILE* f, long v) {
  const int32_t x = (int32_t)v;
  fwrite(&x, 4, 1, f);
}
static cv::Mat pose_mat(const float* T) {
  cv::Mat M = cv::Mat::eye(4, 4, CV_32F);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) M.at<float>(r, c) = T[4 * r + c];
  return M;
}
static void wr_pose(FILE* f, const cv::Mat& M) {
  float T[12] = {0};
  wr32(f, M.rows);
  if (M.rows == 4)
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) T[4 * r + c] = M.at<float>(r, c);
  fwrite(T, 4, 12, f);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  auto get = [fi](void* p, size_t n) {
    if (fread(p, 1, n, fi) != n) {
      fprintf(stderr, "short input\n");
      exit(2);
    }
  };
  int32_t nLoopKF = 0, NK = 0, NM = 0;
  float mb = 0;
  get(&nLoopKF, 4);
  get(&mb, 4);
  get(&NK, 4);
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<MapPoint>> mps;
  Map map;
  std::vector<int32_t> parent(NK);
  for (int k = 0; k < NK; k++) {
    kfs.emplace_back(new KeyFrame());
    KeyFrame& K = *kfs.back();
    int32_t optimised = 0;
    float T[12], G[12];
    get(&parent[k], 4);
    get(&optimised, 4);
    get(T, 48);
    get(G, 48);
    K.mnId = (long unsigned int)k;
    K.mb = mb;
    K.SetPose(pose_mat(T));
    K.set_pose_calls = 0;
    if (optimised) {
      K.mTcwGBA = pose_mat(G);
      K.mnBAGlobalForKF = (long unsigned int)nLoopKF;
    }
  }
  for (int k = 0; k < NK; k++) {
    if (parent[k] < 0)
      map.mvpKeyFrameOrigins.push_back(kfs[k].get());
    else
      kfs[parent[k]]->mspChildrens.insert(kfs[k].get());
  }
  get(&NM, 4);
  for (int m = 0; m < NM; m++) {
    mps.emplace_back(new MapPoint());
    MapPoint& M = *mps.back();
    int32_t bad = 0, optimised = 0, ref = -1;
    float X[3], GX[3];
    get(&bad, 4);
    get(&optimised, 4);
    get(&ref, 4);
    get(X, 12);
    get(GX, 12);
    M.bad = bad != 0;
    M.mpRefKF = ref >= 0 ? kfs[ref].get() : nullptr;
    M.pos = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) M.pos.at<float>(r) = X[r];
    if (optimised) {
      M.mPosGBA = cv::Mat(3, 1, CV_32F);
      for (int r = 0; r < 3; r++) M.mPosGBA.at<float>(r) = GX[r];
      M.mnBAGlobalForKF = (long unsigned int)nLoopKF;
    }
    map.points.push_back(&M);
  }
  fclose(fi);
  const int rc = orbfe_host::RunGlobalBundleAdjustmentUpdateMap(&map, (unsigned long)nLoopKF);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  wr32(fo, rc);
  for (auto& K : kfs) {
    wr32(fo, K->set_pose_calls);
    float T[12];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) T[4 * r + c] = K->Tcw.at<float>(r, c);
    fwrite(T, 4, 12, fo);
    wr32(fo, (long)K->mnBAGlobalForKF);
    wr_pose(fo, K->mTcwGBA);
    wr_pose(fo, K->mTcwBefGBA);
  }
  for (auto& M : mps) {
    wr32(fo, M->set_pos_calls);
    wr32(fo, M->update_calls);
    float X[3];
    for (int r = 0; r < 3; r++) X[r] = M->pos.at<float>(r);
    fwrite(X, 4, 3, fo);
  }
  fclose(fo);
  return 0;
}
