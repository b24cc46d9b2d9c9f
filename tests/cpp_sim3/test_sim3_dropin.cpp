// test_sim3_dropin.cpp -- orbfe_host::Sim3Solver (csrc/host/Sim3Solver_hip.h) on the mock KeyFrame / MapPoint of this directory.
//   test_sim3_dropin <in.bin> <out.bin>
// in.bin  (written by tests/test_sim3_dropin_cpp.py): int32 S, int32 mode (0: find per solver, 1: iterate(5) round-robin as
//         LoopClosing::ComputeSim3 does), uint32 seed of srand, int32 minInliers, int32 maxIterations, then S solvers, each int32
//         fix_scale, two keyframes (orbfe_sim3_view 64 bytes, int32 n_kp, n_kp int32 octaves, int32 n_levels, n_levels float
//         mvLevelSigma2), int32 N1, N1 matches (int32 matched, has_mp1, bad1, bad2, idx1, idx2; float Xw1[3], Xw2[3])
// out.bin: one record per iterate / find call: int32 solver, int32 returned-a-matrix, 16 floats T12 (zeros without), int32 nInliers,
//          int32 bNoMore, int32 N1, N1 bytes vbInliers; then per solver int32 -1, int32 N, int32 mRansacMaxIts, int32 status, float s,
//          9 floats R, 3 floats t (zeros without a best), int32 number of triples, the triples
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "mock/KeyFrame.h"
#include "../../refactored_orb_slam2_amd/csrc/host/Sim3Solver_hip.h"

using namespace ORB_SLAM2;
typedef orbfe_host::Sim3Solver<KeyFrame, MapPoint> Solver;

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
  std::vector<int32_t> oct(n_kp);
  rd(f, oct.data(), n_kp);
  K.mvKeysUn.resize(n_kp);
  for (int i = 0; i < n_kp; i++) K.mvKeysUn[i].octave = oct[i];
  rd(f, &n_levels, 1);
  K.mvLevelSigma2.resize(n_levels);
  rd(f, K.mvLevelSigma2.data(), n_levels);
}

struct Problem {
  KeyFrame kf1, kf2;
  std::vector<std::unique_ptr<MapPoint>> owned;
  std::vector<MapPoint*> matched12;
  std::unique_ptr<Solver> solver;
};

static void write_call(FILE* out, int k, const cv::Mat& T, int nInliers, bool bNoMore, const std::vector<bool>& vb) {
  const int32_t head[2] = {k, !T.empty()};
  float t[16] = {0};
  if (!T.empty())
    for (int i = 0; i < 16; i++) t[i] = T.at<float>(i / 4, i % 4);
  const int32_t tail[3] = {nInliers, bNoMore, (int32_t)vb.size()};
  wr(out, head, 2);
  wr(out, t, 16);
  wr(out, tail, 3);
  for (size_t i = 0; i < vb.size(); i++) fputc(vb[i] ? 1 : 0, out);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t S = 0, mode = 0, min_inliers = 0, max_its = 0;
  uint32_t seed = 0;
  rd(f, &S, 1); rd(f, &mode, 1); rd(f, &seed, 1); rd(f, &min_inliers, 1); rd(f, &max_its, 1);
  std::vector<std::unique_ptr<Problem>> P;
  for (int k = 0; k < S; k++) {
    P.emplace_back(new Problem());
    Problem& p = *P.back();
    int32_t fix = 0, N1 = 0;
    rd(f, &fix, 1);
    read_keyframe(f, p.kf1);
    read_keyframe(f, p.kf2);
    rd(f, &N1, 1);
    p.kf1.mvpMapPoints.assign(N1, nullptr);
    p.matched12.assign(N1, nullptr);
    for (int i = 0; i < N1; i++) {
      int32_t m[6];
      float X[6];
      rd(f, m, 6);
      rd(f, X, 6);
      if (m[1]) {
        p.owned.emplace_back(new MapPoint());
        MapPoint* a = p.owned.back().get();
        a->bad = m[2] != 0;
        a->pos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) a->pos.at<float>(r) = X[r];
        if (m[4] >= 0) a->observations[&p.kf1] = m[4];
        p.kf1.mvpMapPoints[i] = a;
      }
      if (m[0]) {
        p.owned.emplace_back(new MapPoint());
        MapPoint* b = p.owned.back().get();
        b->bad = m[3] != 0;
        b->pos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) b->pos.at<float>(r) = X[3 + r];
        if (m[5] >= 0) b->observations[&p.kf2] = m[5];
        p.matched12[i] = b;
      }
    }
    p.solver.reset(new Solver(&p.kf1, &p.kf2, p.matched12, fix != 0));
    p.solver->SetRansacParameters(0.99, min_inliers, max_its);
  }
  fclose(f);
  srand(seed);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  std::vector<bool> vb;
  int nInliers = 0;
  if (mode == 0) {
    for (int k = 0; k < S; k++) {
      const cv::Mat T = P[k]->solver->find(vb, nInliers);
      write_call(out, k, T, nInliers, false, vb);
    }
  } else {
    std::vector<bool> discarded(S, false);   // LoopClosing.cc:268-330
    int left = S;
    bool matched = false;
    while (left > 0 && !matched) {
      for (int k = 0; k < S; k++) {
        if (discarded[k]) continue;
        bool bNoMore = false;
        const cv::Mat T = P[k]->solver->iterate(5, bNoMore, vb, nInliers);
        write_call(out, k, T, nInliers, bNoMore, vb);
        if (bNoMore) {
          discarded[k] = true;
          left--;
        }
        if (!T.empty()) {
          matched = true;
          break;
        }
      }
    }
  }
  for (int k = 0; k < S; k++) {
    Solver& s = *P[k]->solver;
    const int32_t head[4] = {-1, s.NumCorrespondences(), s.MaxIterations(), s.Status()};
    wr(out, head, 4);
    float v[13] = {0};
    const cv::Mat R = s.GetEstimatedRotation(), t = s.GetEstimatedTranslation();
    v[0] = s.GetEstimatedScale();
    if (!R.empty()) {
      for (int i = 0; i < 9; i++) v[1 + i] = R.at<float>(i / 3, i % 3);
      for (int i = 0; i < 3; i++) v[10 + i] = t.at<float>(i);
    }
    wr(out, v, 13);
    const int32_t nt = (int32_t)(s.Triples().size() / 3);
    wr(out, &nt, 1);
    wr(out, s.Triples().data(), s.Triples().size());
  }
  fclose(out);
  return 0;
}
