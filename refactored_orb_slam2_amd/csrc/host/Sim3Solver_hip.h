// Sim3Solver_hip.h -- host-side adapter with the public surface of ORB_SLAM2::Sim3Solver on liborbfe.
//
// The reference's class (Source/Libraries/ORB_SLAM2/src/Sim3Solver.cc) draws three correspondences, solves Horn's closed form and
// counts inliers, one hypothesis after the other, on the host.  This class keeps the constructor's filtering (:62-100) and the
// `size_t` truncation of the error bounds (:85-86), and on the FIRST iterate() draws all mRansacMaxIts triples with rand() through
// the reference's RandomInt formula (ThirdParty/DLib/DLib-local/src/DUtils/Random.cpp:47-50) and the swap-with-back sampling of
// :159-172, evaluates them in ONE orbfe_sim3_solve call (include/orbfe.h) and afterwards serves iterate(n) from the stored counts
// with a cursor: same `>=` update of the best hypothesis, same return on `> mRansacMinInliers`, bNoMore on the call that consumes
// iteration mRansacMaxIts without returning (refactored_orb_slam2_amd/sim3.py: iterate_replay is the same cursor in Python).
//
// Deviation from the reference: it draws lazily, three rand() calls per iteration it actually runs.  With several solvers
// interleaved on one rand() stream (LoopClosing::ComputeSim3 runs iterate(5) round-robin over its candidates) each solver here
// consumes its whole budget of draws at its first iterate(), so it sees a different subsequence of the stream than it would there.
// The distribution of the triples is the same; the sequence is not.
//
// A template over the KeyFrame and MapPoint types so that it compiles (and is unit-tested, tests/cpp_sim3) without the reference
// tree.  A failing library call is logged to stderr, never thrown: the solver then reports bNoMore and returns empty matrices.
//
// Members used (same names as the reference):
//   KeyFrame: GetMapPointMatches(), GetRotation(), GetTranslation(), mvKeysUn, mvLevelSigma2, mK
//   MapPoint: isBad(), GetIndexInKeyFrame(pKF), GetWorldPos()
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../../include/orbfe.h"
#ifdef ORBFE_HAVE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvlite.h"
#endif

namespace ORB_SLAM2 {
namespace orbfe_host {

template <class KeyFrameT>
inline orbfe_sim3_view MakeSim3View(KeyFrameT* pKF) {
  orbfe_sim3_view v;
  memset(&v, 0, sizeof(v));
  const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation();
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) v.Rcw[3 * r + c] = R.template at<float>(r, c);
    v.tcw[r] = t.template at<float>(r);
  }
  v.fx = pKF->mK.template at<float>(0, 0); v.fy = pKF->mK.template at<float>(1, 1);
  v.cx = pKF->mK.template at<float>(0, 2); v.cy = pKF->mK.template at<float>(1, 2);
  return v;
}

// DUtils::Random::RandomInt(min, max) on rand()
inline int RandomInt(int min, int max) {
  const int d = max - min + 1;
  return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

template <class KeyFrameT, class MapPointT>
class Sim3Solver {
 public:
  Sim3Solver(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true)
      : mbFixScale(bFixScale) {
    std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = (int)vpMatched12.size();
    mView1 = MakeSim3View(pKF1);
    mView2 = MakeSim3View(pKF2);
    for (int i1 = 0; i1 < mN1; i1++) {   // :62-100
      if (!vpMatched12[i1]) continue;
      MapPointT* pMP1 = vpKeyFrameMP1[i1];
      MapPointT* pMP2 = vpMatched12[i1];
      if (!pMP1) continue;
      if (pMP1->isBad() || pMP2->isBad()) continue;
      const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
      if (indexKF1 < 0 || indexKF2 < 0) continue;
      const float sigmaSquare1 = pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave];
      const float sigmaSquare2 = pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave];
      orbfe_sim3_pair p;
      const cv::Mat X1 = pMP1->GetWorldPos(), X2 = pMP2->GetWorldPos();
      for (int r = 0; r < 3; r++) {
        p.Xw1[r] = X1.template at<float>(r);
        p.Xw2[r] = X2.template at<float>(r);
      }
      p.max_err1 = (float)(size_t)(9.210 * sigmaSquare1);   // vector<size_t>::push_back(double), read back by a float comparison
      p.max_err2 = (float)(size_t)(9.210 * sigmaSquare2);
      mvPairs.push_back(p);
      mvnIndices1.push_back((size_t)i1);
    }
    SetRansacParameters();
  }

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    N = (int)mvPairs.size();
    mRansacMaxIts = std::max(maxIterations, 1);
    if (N >= 1 && minInliers >= 0 && minInliers <= N) {
      const int its = orbfe_sim3_ransac_iterations(N, probability, minInliers, maxIterations);
      if (its >= 1) mRansacMaxIts = its;
    }
    mnIterations = 0;
    mbSolved = false;
    mnBest = -1;
    mnBestInliers = 0;
  }

  cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
  }

  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (N < mRansacMinInliers || N < 3) {   // :144-147 (fewer than three correspondences cannot be sampled at all)
      bNoMore = true;
      return cv::Mat();
    }
    if (!mbSolved && !Solve()) {
      bNoMore = true;
      return cv::Mat();
    }
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
      nCurrentIterations++;
      const int h = mnIterations++;
      const int c = mvHyps[h].n_inliers;
      if (c >= mnBestInliers) {   // :178-185
        mnBest = h;
        mnBestInliers = c;
        if (c > mRansacMinInliers) {
          nInliers = c;
          const uint64_t* row = mvWords.data() + (size_t)h * mnWords;
          for (int i = 0; i < N; i++)
            if ((row[i >> 6] >> (i & 63)) & 1) vbInliers[mvnIndices1[i]] = true;
          return BestT12();
        }
      }
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return cv::Mat();
  }

  cv::Mat GetEstimatedRotation() {
    if (mnBest < 0) return cv::Mat();
    cv::Mat R(3, 3, CV_32F);
    for (int i = 0; i < 9; i++) R.template at<float>(i / 3, i % 3) = mvHyps[mnBest].R[i];
    return R;
  }
  cv::Mat GetEstimatedTranslation() {
    if (mnBest < 0) return cv::Mat();
    cv::Mat t(3, 1, CV_32F);
    for (int i = 0; i < 3; i++) t.template at<float>(i) = mvHyps[mnBest].t[i];
    return t;
  }
  float GetEstimatedScale() { return mnBest < 0 ? 0.f : mvHyps[mnBest].s; }

  // beyond the reference's surface: what the solver was built from and what the library answered
  int NumCorrespondences() const { return N; }
  int MaxIterations() const { return mRansacMaxIts; }
  int Status() const { return mnStatus; }
  const std::vector<int32_t>& Triples() const { return mvTriples; }

 private:
  bool Solve() {
    mvTriples.resize((size_t)mRansacMaxIts * 3);
    std::vector<int32_t> vAvailableIndices;
    for (int it = 0; it < mRansacMaxIts; it++) {   // :159-172
      vAvailableIndices.resize(N);
      for (int i = 0; i < N; i++) vAvailableIndices[i] = i;
      for (short i = 0; i < 3; ++i) {
        const int randi = RandomInt(0, (int)vAvailableIndices.size() - 1);
        mvTriples[(size_t)it * 3 + i] = vAvailableIndices[randi];
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
    mnWords = (N + 63) / 64;
    mvHyps.assign(mRansacMaxIts, orbfe_sim3_hypothesis());
    mvWords.assign((size_t)mRansacMaxIts * mnWords, 0);
    std::vector<uint64_t> mask(mnWords);
    orbfe_sim3_result res;
    mnStatus = orbfe_sim3_solve(&mView1, &mView2, mvPairs.data(), N, mvTriples.data(), mRansacMaxIts, mbFixScale ? 1 : 0, mRansacMinInliers,
                                mvHyps.data(), mvWords.data(), &res, mask.data());
    if (mnStatus != ORBFE_OK) {
      fprintf(stderr, "Sim3Solver: orbfe_sim3_solve failed with %d: %s\n", mnStatus, orbfe_last_error());
      return false;
    }
    mbSolved = true;
    return true;
  }

  cv::Mat BestT12() {   // :306-311
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    const orbfe_sim3_hypothesis& h = mvHyps[mnBest];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T.template at<float>(r, c) = h.s * h.R[3 * r + c];
      T.template at<float>(r, 3) = h.t[r];
    }
    return T;
  }

  orbfe_sim3_view mView1, mView2;
  std::vector<orbfe_sim3_pair> mvPairs;
  std::vector<size_t> mvnIndices1;
  std::vector<int32_t> mvTriples;
  std::vector<orbfe_sim3_hypothesis> mvHyps;
  std::vector<uint64_t> mvWords;
  int mN1 = 0, N = 0, mnWords = 0;
  bool mbFixScale, mbSolved = false;
  double mRansacProb = 0.99;
  int mRansacMinInliers = 6, mRansacMaxIts = 300, mnIterations = 0, mnBest = -1, mnBestInliers = 0, mnStatus = ORBFE_OK;
};

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
