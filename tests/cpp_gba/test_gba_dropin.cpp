// test_gba_dropin.cpp -- orbfe_host::GlobalBundleAdjustemnt (csrc/host/Optimizer_hip.h) on a mock map of more than 64 keyframes,
// which the adapter, compiled with ORBFE_HOST_GLOBAL_BA_ACROSS_DEVICE, hands to orbfe_global_bundle_adjustment.  The mocks and the file formats are tests/cpp_ba's:
//   test_gba_dropin <in.bin> <out.bin>
// in.bin  (written by tests/test_gba_dropin_cpp.py): 5 floats fx fy cx cy mbf; int32 n_levels, n_levels float mvInvLevelSigma2;
//         int32 NK, NK keyframes (int32 mnId, int32 bad, 12 floats of [R | t], int32 n_kp, n_kp x (float x, float y, int32 octave,
//         float mvuRight)); int32 NM, NM map points (int32 mnId, int32 bad, 3 floats, int32 n_obs, n_obs x (int32 keyframe index,
//         int32 keypoint)); int32 in_map[NK]; int32 nIterations, int32 bRobust, int32 nLoopKF, int32 stop flag
// out.bin int32 0; NK x (int32 SetPose calls, 12 floats, int32 mnBAGlobalForKF, int32 mTcwGBA rows, 12 floats of it or zeros); NM x
//         (int32 SetWorldPos calls, int32 UpdateNormalAndDepth calls, 3 floats, int32 mnBAGlobalForKF, int32 mPosGBA rows, 3 floats of
//         it or zeros)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "mock/KeyFrame.h"
#include "mock/Map.h"
#define ORBFE_HOST_GLOBAL_BA_ACROSS_DEVICE   // a map beyond the one-workgroup limits goes to orbfe_global_bundle_adjustment
#include "../../refactored_orb_slam2_amd/csrc/host/Optimizer_hip.h"

using namespace ORB_SLAM2;

template <class T>
static void wr(FILE* f, const T* p, size_t n) {
  if (n) fwrite(p, sizeof(T), n, f);
}
static void wr32(FILE* f, long v) {
  const int32_t x = (int32_t)v;
  wr(f, &x, 1);
}

struct Scene {
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<MapPoint>> mps;
  Map map;
  int nIterations = 5, bRobust = 1, nLoopKF = 0, stop = 0;
};

static void build(const std::vector<uint8_t>& raw, Scene& S) {
  size_t off = 0;
  auto get = [&raw, &off](void* p, size_t n) {
    if (off + n > raw.size()) {
      fprintf(stderr, "short input\n");
      exit(2);
    }
    memcpy(p, raw.data() + off, n);
    off += n;
  };
  int32_t n_levels = 0, NK = 0, NM = 0;
  float cam[5];
  get(cam, 20);
  get(&n_levels, 4);
  std::vector<float> sig(n_levels);
  get(sig.data(), 4 * (size_t)n_levels);
  get(&NK, 4);
  for (int k = 0; k < NK; k++) {
    S.kfs.emplace_back(new KeyFrame());
    KeyFrame& K = *S.kfs.back();
    int32_t id = 0, bad = 0, n_kp = 0;
    float T[12];
    get(&id, 4);
    get(&bad, 4);
    get(T, 48);
    K.mnId = (long unsigned int)id;
    K.bad = bad != 0;
    K.Tcw = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) K.Tcw.at<float>(r, c) = T[4 * r + c];
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mbf = cam[4];
    K.mvInvLevelSigma2 = sig;
    get(&n_kp, 4);
    K.N = n_kp;
    K.mvpMapPoints.assign(n_kp, nullptr);
    for (int i = 0; i < n_kp; i++) {
      float x, y, ur;
      int32_t oct;
      get(&x, 4);
      get(&y, 4);
      get(&oct, 4);
      get(&ur, 4);
      K.mvKeysUn.push_back(cv::KeyPoint(x, y, 31.f, -1, 0, oct));
      K.mvuRight.push_back(ur);
    }
  }
  get(&NM, 4);
  for (int m = 0; m < NM; m++) {
    S.mps.emplace_back(new MapPoint());
    MapPoint& M = *S.mps.back();
    int32_t id = 0, bad = 0, n_obs = 0;
    float X[3];
    get(&id, 4);
    get(&bad, 4);
    get(X, 12);
    M.mnId = (long unsigned int)id;
    M.bad = bad != 0;
    M.pos = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) M.pos.at<float>(r) = X[r];
    get(&n_obs, 4);
    for (int o = 0; o < n_obs; o++) {
      int32_t kf, kp;
      get(&kf, 4);
      get(&kp, 4);
      M.observations[S.kfs[kf].get()] = (size_t)kp;
      S.kfs[kf]->mvpMapPoints[kp] = &M;
    }
    S.map.points.push_back(&M);
  }
  for (int k = 0; k < NK; k++) {
    int32_t in_map = 0;
    get(&in_map, 4);
    if (in_map) S.map.keyframes.push_back(S.kfs[k].get());
  }
  int32_t v[4];
  get(v, 16);
  S.nIterations = v[0]; S.bRobust = v[1]; S.nLoopKF = v[2]; S.stop = v[3];
}

static void dump_map(FILE* f, Scene& S) {
  const float zeros[12] = {0};
  for (auto& K : S.kfs) {
    wr32(f, K->set_pose_calls);
    float T[12];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) T[4 * r + c] = K->Tcw.at<float>(r, c);
    wr(f, T, 12);
    wr32(f, (long)K->mnBAGlobalForKF);
    wr32(f, K->mTcwGBA.rows);
    if (K->mTcwGBA.rows == 4) {
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) T[4 * r + c] = K->mTcwGBA.at<float>(r, c);
      wr(f, T, 12);
    } else {
      wr(f, zeros, 12);
    }
  }
  for (auto& M : S.mps) {
    wr32(f, M->set_pos_calls);
    wr32(f, M->update_calls);
    float X[3];
    for (int r = 0; r < 3; r++) X[r] = M->pos.at<float>(r);
    wr(f, X, 3);
    wr32(f, (long)M->mnBAGlobalForKF);
    wr32(f, M->mPosGBA.rows);
    if (M->mPosGBA.rows == 3) {
      for (int r = 0; r < 3; r++) X[r] = M->mPosGBA.at<float>(r);
      wr(f, X, 3);
    } else {
      wr(f, zeros, 3);
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  std::vector<uint8_t> raw;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), fi)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(fi);
  Scene S;
  build(raw, S);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  bool stop = S.stop != 0;
  orbfe_host::GlobalBundleAdjustemnt(&S.map, S.nIterations, &stop, (unsigned long)S.nLoopKF, S.bRobust != 0);
  wr32(fo, 0);
  dump_map(fo, S);
  fclose(fo);
  return 0;
}
