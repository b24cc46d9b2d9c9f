// test_optsim3_dropin.cpp -- orbfe_host::OptimizeSim3 (csrc/host/Optimizer_hip.h) on the mock KeyFrame / MapPoint / Sim3 of this
// directory.
//   test_optsim3_dropin <in.bin> <out.bin>
// in.bin  (written by tests/test_optsim3_dropin_cpp.py): int32 S, then S problems, each int32 fix_scale, float th2, 13 floats
//         s R t, two keyframes (orbfe_sim3_view 64 bytes, int32 n_kp, n_kp x (float x, float y, int32 octave), int32 n_levels,
//         n_levels float mvInvLevelSigma2), int32 N, N matches (int32 matched, has_mp1, bad1, bad2, idx2; float Xw1[3], Xw2[3])
// out.bin: per problem what the adapter marshals (int32 n, n orbfe_optsim3_pair, n int32 vnIndexEdge), then int32 return value, int32 "g2oS12 was written", 13 floats s R t of g2oS12 afterwards, int32 N, N bytes
//          (vpMatches1[i] != NULL afterwards)
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "mock/KeyFrame.h"
#include "../../refactored_orb_slam2_amd/csrc/host/Optimizer_hip.h"

using namespace ORB_SLAM2;

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
}
template <class T>
static void wr(FILE* f, const T* p, size_t n) {
  if (n) fwrite(p, sizeof(T), n, f);
}

static void read_keyframe(FILE* f, KeyFrame& K) {
  orbfe_sim3_view v;
  rd(f, &v, 1);
  K.Rcw = cv::Mat(3, 3, CV_32F);
  K.tcw = cv::Mat(3, 1, CV_32F);
  K.mK = cv::Mat::eye(3, 3, CV_32F);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) K.Rcw.at<float>(r, c) = v.Rcw[3 * r + c];
    K.tcw.at<float>(r) = v.tcw[r];
  }
  K.mK.at<float>(0, 0) = v.fx; K.mK.at<float>(1, 1) = v.fy; K.mK.at<float>(0, 2) = v.cx; K.mK.at<float>(1, 2) = v.cy;
  int32_t n_kp = 0, n_levels = 0;
  rd(f, &n_kp, 1);
  K.mvKeysUn.resize(n_kp);
  for (int i = 0; i < n_kp; i++) {
    float xy[2];
    int32_t oct;
    rd(f, xy, 2);
    rd(f, &oct, 1);
    K.mvKeysUn[i].pt.x = xy[0];
    K.mvKeysUn[i].pt.y = xy[1];
    K.mvKeysUn[i].octave = oct;
  }
  rd(f, &n_levels, 1);
  K.mvInvLevelSigma2.resize(n_levels);
  rd(f, K.mvInvLevelSigma2.data(), n_levels);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!f || !out) return 2;
  int32_t S = 0;
  rd(f, &S, 1);
  for (int k = 0; k < S; k++) {
    int32_t fix = 0, N = 0;
    float th2 = 0, v[13];
    rd(f, &fix, 1);
    rd(f, &th2, 1);
    rd(f, v, 13);
    KeyFrame kf1, kf2;
    read_keyframe(f, kf1);
    read_keyframe(f, kf2);
    rd(f, &N, 1);
    std::vector<std::unique_ptr<MapPoint>> owned;
    std::vector<MapPoint*> vpMatches1(N, nullptr);
    kf1.mvpMapPoints.assign(N, nullptr);
    for (int i = 0; i < N; i++) {
      int32_t m[5];
      float X[6];
      rd(f, m, 5);
      rd(f, X, 6);
      if (m[1]) {
        owned.emplace_back(new MapPoint());
        MapPoint* a = owned.back().get();
        a->bad = m[2] != 0;
        a->pos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) a->pos.at<float>(r) = X[r];
        kf1.mvpMapPoints[i] = a;
      }
      if (m[0]) {
        owned.emplace_back(new MapPoint());
        MapPoint* b = owned.back().get();
        b->bad = m[3] != 0;
        b->pos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) b->pos.at<float>(r) = X[3 + r];
        if (m[4] >= 0) b->observations[&kf2] = m[4];
        vpMatches1[i] = b;
      }
    }
    mockg2o::Matrix3 R;
    mockg2o::Vector3 t;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R(r, c) = v[1 + 3 * r + c];
      t[r] = v[10 + r];
    }
    mockg2o::Sim3 g2oS12(R, t, v[0]);
    g2oS12.constructed = 0;
    {
      orbfe_sim3_view v1, v2;
      std::vector<orbfe_optsim3_pair> pairs;
      std::vector<size_t> index;
      orbfe_host::OptimizeSim3Marshal(&kf1, &kf2, vpMatches1, v1, v2, pairs, index);
      const int32_t n = (int32_t)pairs.size();
      wr(out, &n, 1);
      wr(out, pairs.data(), pairs.size());
      for (size_t e = 0; e < index.size(); e++) {
        const int32_t ix = (int32_t)index[e];
        wr(out, &ix, 1);
      }
    }
    const int ret = orbfe_host::OptimizeSim3(&kf1, &kf2, vpMatches1, g2oS12, th2, fix != 0);
    const int32_t head[2] = {ret, g2oS12.constructed};
    wr(out, head, 2);
    float o[13];
    o[0] = (float)g2oS12.scale();
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) o[1 + 3 * r + c] = (float)g2oS12.rotation().toRotationMatrix()(r, c);
      o[10 + r] = (float)g2oS12.translation()[r];
    }
    wr(out, o, 13);
    wr(out, &N, 1);
    for (int i = 0; i < N; i++) fputc(vpMatches1[i] ? 1 : 0, out);
  }
  fclose(f);
  fclose(out);
  return 0;
}
