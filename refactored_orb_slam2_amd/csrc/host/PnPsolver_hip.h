// PnPsolver_hip.h -- host-side adapter with the public surface of ORB_SLAM2::PnPsolver on liborbfe.
//
// The reference's class (Source/Libraries/ORB_SLAM2/src/PnPsolver.cc) draws four correspondences, solves EPnP, counts inliers and
// refines the best hypothesis so far, one iteration after the other, on the host.  This class keeps the constructor's filtering
// (:81-101) and SetRansacParameters (:119-156, through orbfe_pnp_ransac_parameters), draws the minimal sets of ALL its iterations
// with the swap-with-back sampling of :184-197, has them evaluated by the device -- SolveAll() takes every candidate of a
// relocalisation in ONE orbfe_pnp_solve_batch_device call -- and afterwards serves iterate(n) from the stored counts and refine
// records with a cursor: same `||` loop condition, same `>=` / `>` tests, same Refine() on the best so far, bNoMore once mnIterations
// has reached mRansacMaxIts (refactored_orb_slam2_amd/pnp.py: iterate_replay is the same cursor in Python).  A solver that
// SolveAll() has not seen solves itself at its first iterate().
//
// Deviations from the reference:
//   - it draws lazily, four random numbers per iteration it actually runs; here a solver consumes the draws of its whole budget
//     (mRansacMaxIts iterations plus ExtraIterations, the room for one more iterate(5) behind the budget) when it is solved.  The
//     distribution of the sets is the same; the sequence on a shared stream is not.  An iterate() that walks past the evaluated
//     hypotheses draws more and solves again (every earlier record comes back identical: a record depends on its set only);
//   - the random numbers come from a caller-supplied generator (SetRandom: k -> integer in [0, k)), by default the reference's
//     RandomInt formula on rand() (ThirdParty/DLib/DLib-local/src/DUtils/Random.cpp:47-50);
//   - the null-space basis of a minimal solve is this library's (include/orbfe.h, the PnPsolver block).
//
// A template over the Frame and MapPoint types so that it compiles (and is unit-tested, tests/cpp_pnp) without the reference tree.
// A failing library call is logged to stderr, never thrown: the solver then reports bNoMore and returns empty matrices.
//
// Members used (same names as the reference):
//   Frame:    mvKeysUn, mvLevelSigma2, fx, fy, cx, cy
//   MapPoint: isBad(), GetWorldPos()
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../../../include/orbfe.h"
#ifdef ORBFE_HAVE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvlite.h"
#endif

namespace ORB_SLAM2 {
namespace orbfe_host {

// DUtils::Random::RandomInt(0, k - 1) on rand()
inline int PnPRandomBelow(int k) { return int(((double)rand() / ((double)RAND_MAX + 1.0)) * k); }

template <class FrameT, class MapPointT>
class PnPsolver {
 public:
  PnPsolver(const FrameT& F, const std::vector<MapPointT*>& vpMapPointMatches) : mnMatches((int)vpMapPointMatches.size()) {
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {   // :81-101
      MapPointT* pMP = vpMapPointMatches[i];
      if (!pMP || pMP->isBad()) continue;
      const cv::KeyPoint& kp = F.mvKeysUn[i];
      orbfe_pnp_point p;
      const cv::Mat Pos = pMP->GetWorldPos();
      for (int r = 0; r < 3; r++) p.Xw[r] = Pos.template at<float>(r);
      p.u = kp.pt.x;
      p.v = kp.pt.y;
      p.max_err = 0.f;
      mvPoints.push_back(p);
      mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
      mvKeyPointIndices.push_back(i);
    }
    mCamera.fx = F.fx; mCamera.fy = F.fy; mCamera.cx = F.cx; mCamera.cy = F.cy;
    SetRansacParameters();
  }

  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                           float th2 = 5.991) {
    N = (int)mvPoints.size();
    mRansacMinInliers = std::max(minInliers, minSet);
    mRansacMaxIts = std::max(maxIterations, 1);
    mnStatus = ORBFE_OK;
    if (N >= 1) {
      int32_t mi = 0, its = 0;
      float eps = 0.f;
      mnStatus = orbfe_pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mi, &its, &eps);
      if (mnStatus == ORBFE_OK) {
        mRansacMinInliers = mi;
        mRansacMaxIts = its;
      } else {
        fprintf(stderr, "PnPsolver: orbfe_pnp_ransac_parameters failed with %d: %s\n", mnStatus, orbfe_last_error());
      }
    }
    for (int i = 0; i < N; i++) mvPoints[i].max_err = mvSigma2[i] * th2;   // :155
    mnIterations = 0;
    mnBest = -1;
    mnBestInliers = 0;
    mvSets.clear();
    mnSolved = 0;
  }

  // k -> an integer in [0, k); the default is the reference's RandomInt on rand()
  void SetRandom(std::function<int(int)> below) { mBelow = below; }
  // iterations evaluated behind mRansacMaxIts at the first solve: one more iterate(5) may run there (the `||` of :179)
  void SetExtraIterations(int n) { mnExtra = std::max(n, 0); }

  cv::Mat find(std::vector<bool>& vbInliers, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
  }

  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (N < mRansacMinInliers || mnStatus != ORBFE_OK) {   // :171-174
      bNoMore = true;
      return cv::Mat();
    }
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {
      if (mnIterations >= mnSolved) {   // the first call, or a walk past what has been evaluated
        std::vector<PnPsolver*> self(1, this);
        const int want = std::max(mnIterations + (nIterations - nCurrentIterations), mRansacMaxIts + mnExtra);
        if (!Solve(self, want)) {
          bNoMore = true;
          return cv::Mat();
        }
      }
      nCurrentIterations++;
      const int h = mnIterations++;
      const int c = mvHyps[h].n_inliers;
      if (c >= mRansacMinInliers) {
        if (c > mnBestInliers) {   // :207-218
          mnBest = h;
          mnBestInliers = c;
        }
        const orbfe_pnp_refine& r = mvRefines[mnBest];   // Refine() on the best so far (:220, :248-289)
        if (r.n_inliers > mRansacMinInliers) {
          nInliers = r.n_inliers;
          Inliers(mvRefineWords.data() + (size_t)mnBest * mnWords, vbInliers);
          return Pose(r.R, r.t);
        }
      }
    }
    if (mnIterations >= mRansacMaxIts) {   // :232-243
      bNoMore = true;
      if (mnBestInliers >= mRansacMinInliers) {
        nInliers = mnBestInliers;
        Inliers(mvWords.data() + (size_t)mnBest * mnWords, vbInliers);
        return Pose(mvHyps[mnBest].R, mvHyps[mnBest].t);
      }
    }
    return cv::Mat();
  }

  // Every candidate of a relocalisation in one batch call (Tracking.cc:1258-1283 builds the solvers, then :1298 iterates them).
  // Solvers with N < mRansacMinInliers are left alone.  Returns ORBFE_OK or the failing call's code (also kept in Status()).
  static int SolveAll(std::vector<PnPsolver*>& solvers) {
    std::vector<PnPsolver*> live;
    for (size_t i = 0; i < solvers.size(); i++)
      if (solvers[i] && solvers[i]->N >= solvers[i]->mRansacMinInliers && solvers[i]->N >= 4 && solvers[i]->mnStatus == ORBFE_OK)
        live.push_back(solvers[i]);
    if (live.empty()) return ORBFE_OK;
    return Solve(live, 0) ? ORBFE_OK : live[0]->mnStatus;
  }

  // beyond the reference's surface: what the solver was built from and what the library answered
  int NumCorrespondences() const { return N; }
  int MinInliers() const { return mRansacMinInliers; }
  int MaxIterations() const { return mRansacMaxIts; }
  int Iterations() const { return mnIterations; }
  int Status() const { return mnStatus; }
  const std::vector<int32_t>& Sets() const { return mvSets; }
  const std::vector<orbfe_pnp_point>& Points() const { return mvPoints; }
  const std::vector<size_t>& KeyPointIndices() const { return mvKeyPointIndices; }

 private:
  void Draw(int total) {   // :184-197 for iterations [drawn, total)
    std::vector<int32_t> vAvailableIndices;
    for (int it = (int)mvSets.size() / 4; it < total; it++) {
      vAvailableIndices.resize(N);
      for (int i = 0; i < N; i++) vAvailableIndices[i] = i;
      for (short i = 0; i < 4; ++i) {
        int randi = mBelow ? mBelow((int)vAvailableIndices.size()) : PnPRandomBelow((int)vAvailableIndices.size());
        randi = std::min(std::max(randi, 0), (int)vAvailableIndices.size() - 1);
        mvSets.push_back(vAvailableIndices[randi]);
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
  }

  static bool Fail(std::vector<PnPsolver*>& v, int rc, const char* what) {
    fprintf(stderr, "PnPsolver: %s failed with %d: %s\n", what, rc, orbfe_last_error());
    for (size_t i = 0; i < v.size(); i++) v[i]->mnStatus = rc;
    return false;
  }

  // draws what is missing up to max(want, budget) per solver and evaluates all sets of all solvers in one batch call
  static bool Solve(std::vector<PnPsolver*>& v, int want) {
    const int P = (int)v.size();
    int cap = 1, h_cap = 1;
    for (int k = 0; k < P; k++) {
      v[k]->Draw(std::max(want, v[k]->mRansacMaxIts + v[k]->mnExtra));
      cap = std::max(cap, v[k]->N);
      h_cap = std::max(h_cap, (int)v[k]->mvSets.size() / 4);
    }
    if (cap > ORBFE_PNP_MAX_POINTS || h_cap > ORBFE_PNP_MAX_HYPOTHESES) {
      fprintf(stderr, "PnPsolver: %d correspondences or %d hypotheses are beyond the library's limits\n", cap, h_cap);
      for (int k = 0; k < P; k++) v[k]->mnStatus = ORBFE_ERR_INVALID;
      return false;
    }
    int ndev = 0;
    if (orbfe_device_count(&ndev) != ORBFE_OK || ndev < 1) {
      fprintf(stderr, "PnPsolver: no HIP device available (liborbfe has no CPU fallback)\n");
      for (int k = 0; k < P; k++) v[k]->mnStatus = ORBFE_ERR_NO_DEVICE;
      return false;
    }
    const size_t W = ((size_t)cap + 63) / 64;
    // one block: inputs, then outputs
    size_t off = 0;
    auto region = [&off](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_cam = region((size_t)P * sizeof(orbfe_pnp_camera)), o_pts = region((size_t)P * cap * sizeof(orbfe_pnp_point)),
                 o_n = region((size_t)P * 4), o_sets = region((size_t)P * h_cap * 16), o_H = region((size_t)P * 4), o_mi = region((size_t)P * 4),
                 in_end = off;
    const size_t o_hyps = region((size_t)P * h_cap * sizeof(orbfe_pnp_hypothesis)), o_words = region((size_t)P * h_cap * W * 8),
                 o_ref = region((size_t)P * h_cap * sizeof(orbfe_pnp_refine)), o_rwords = region((size_t)P * h_cap * W * 8),
                 o_res = region((size_t)P * sizeof(orbfe_pnp_result)), o_mask = region((size_t)P * W * 8), total = off;
    std::vector<uint8_t> host(total, 0);
    for (int k = 0; k < P; k++) {
      PnPsolver& s = *v[k];
      const int32_t n = s.N, H = (int32_t)s.mvSets.size() / 4, mi = s.mRansacMinInliers;
      memcpy(&host[o_cam + (size_t)k * sizeof(orbfe_pnp_camera)], &s.mCamera, sizeof(orbfe_pnp_camera));
      memcpy(&host[o_pts + (size_t)k * cap * sizeof(orbfe_pnp_point)], s.mvPoints.data(), (size_t)n * sizeof(orbfe_pnp_point));
      memcpy(&host[o_sets + (size_t)k * h_cap * 16], s.mvSets.data(), (size_t)H * 16);
      memcpy(&host[o_n + (size_t)k * 4], &n, 4);
      memcpy(&host[o_H + (size_t)k * 4], &H, 4);
      memcpy(&host[o_mi + (size_t)k * 4], &mi, 4);
    }
    void* d = nullptr;
    int rc = orbfe_device_malloc(total, &d);
    if (rc != ORBFE_OK) return Fail(v, rc, "orbfe_device_malloc");
    uint8_t* D = (uint8_t*)d;
    rc = orbfe_device_upload(D, host.data(), total);   // the whole block: refine rows the kernels skip stay zero
    if (rc == ORBFE_OK)
      rc = orbfe_pnp_solve_batch_device(P, (const orbfe_pnp_camera*)(D + o_cam), (const orbfe_pnp_point*)(D + o_pts), (const int32_t*)(D + o_n),
                                        cap, (const int32_t*)(D + o_sets), (const int32_t*)(D + o_H), h_cap, (const int32_t*)(D + o_mi),
                                        (orbfe_pnp_hypothesis*)(D + o_hyps), (uint64_t*)(D + o_words), (orbfe_pnp_refine*)(D + o_ref),
                                        (uint64_t*)(D + o_rwords), nullptr, nullptr, (orbfe_pnp_result*)(D + o_res), (uint64_t*)(D + o_mask),
                                        nullptr);
    if (rc == ORBFE_OK) rc = orbfe_device_download(&host[in_end], D + in_end, total - in_end);   // a copy on the NULL stream: behind the kernels
    orbfe_device_free(d);
    if (rc != ORBFE_OK) return Fail(v, rc, "orbfe_pnp_solve_batch_device");
    for (int k = 0; k < P; k++) {
      PnPsolver& s = *v[k];
      const size_t H = s.mvSets.size() / 4;
      s.mnWords = (int)(((size_t)s.N + 63) / 64);
      s.mvHyps.resize(H);
      s.mvRefines.resize(H);
      s.mvWords.assign(H * s.mnWords, 0);
      s.mvRefineWords.assign(H * s.mnWords, 0);
      memcpy(s.mvHyps.data(), &host[o_hyps + (size_t)k * h_cap * sizeof(orbfe_pnp_hypothesis)], H * sizeof(orbfe_pnp_hypothesis));
      memcpy(s.mvRefines.data(), &host[o_ref + (size_t)k * h_cap * sizeof(orbfe_pnp_refine)], H * sizeof(orbfe_pnp_refine));
      for (size_t h = 0; h < H; h++) {
        memcpy(&s.mvWords[h * s.mnWords], &host[o_words + ((size_t)k * h_cap + h) * W * 8], (size_t)s.mnWords * 8);
        memcpy(&s.mvRefineWords[h * s.mnWords], &host[o_rwords + ((size_t)k * h_cap + h) * W * 8], (size_t)s.mnWords * 8);
      }
      s.mnSolved = (int)H;
    }
    return true;
  }

  void Inliers(const uint64_t* row, std::vector<bool>& vbInliers) const {   // :222-226, :236-240
    vbInliers = std::vector<bool>(mnMatches, false);
    for (int i = 0; i < N; i++)
      if ((row[i >> 6] >> (i & 63)) & 1) vbInliers[mvKeyPointIndices[i]] = true;
  }

  static cv::Mat Pose(const double* R, const double* t) {   // :211-217, :278-284
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T.template at<float>(r, c) = (float)R[3 * r + c];
      T.template at<float>(r, 3) = (float)t[r];
    }
    return T;
  }

  orbfe_pnp_camera mCamera;
  std::vector<orbfe_pnp_point> mvPoints;
  std::vector<float> mvSigma2;
  std::vector<size_t> mvKeyPointIndices;
  std::vector<int32_t> mvSets;
  std::vector<orbfe_pnp_hypothesis> mvHyps;
  std::vector<orbfe_pnp_refine> mvRefines;
  std::vector<uint64_t> mvWords, mvRefineWords;
  std::function<int(int)> mBelow;
  int mnMatches = 0, N = 0, mnWords = 0, mnSolved = 0, mnExtra = 5;
  int mRansacMinInliers = 8, mRansacMaxIts = 300, mnIterations = 0, mnBest = -1, mnBestInliers = 0, mnStatus = ORBFE_OK;
};

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
