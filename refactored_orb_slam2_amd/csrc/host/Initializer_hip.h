// Initializer_hip.h -- host-side adapter with the public surface of ORB_SLAM2::Initializer on liborbfe.
//
// The reference's class (Source/Libraries/ORB_SLAM2/src/Initializer.cc) keeps the reference frame's keypoints and calibration, and
// Initialize() draws mMaxIterations sets of eight matches, runs FindHomography and FindFundamental on two threads and reconstructs
// from the better model.  This class keeps the constructor and the signature of Initialize(), draws the sets with rand() through
// the reference's RandomInt formula (Sim3Solver_hip.h) and the swap-with-back sampling of :80-93 after seeding rand() once with 0
// (DUtils::Random::SeedRandOnce(0)), and evaluates everything in ONE orbfe_initializer_initialize call (include/orbfe.h).
// rand() is the process's stream, as it is for the reference: the first call's sets, drawn right behind the seeding, are the
// reference's; later ones depend on whatever else in the process drew in between.
//
// A template over the Frame type so that it compiles (and is unit-tested, tests/cpp_initializer) without the reference tree.  A
// failing library call is logged to stderr, never thrown: Initialize() then returns false.  Fewer than 8 matches return false (the
// reference would loop forever drawing from an empty list; Tracking never calls it below 100).
//
// Members used (same names as the reference): Frame::mvKeysUn, Frame::mK
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "Sim3Solver_hip.h"   // RandomInt, cv types, orbfe.h

namespace ORB_SLAM2 {
namespace orbfe_host {

template <class FrameT>
class Initializer {
 public:
  // Fix the reference frame
  Initializer(const FrameT& ReferenceFrame, float sigma = 1.0, int iterations = 200) : mMaxIterations(iterations) {
    memset(&mParams, 0, sizeof(mParams));
    mParams.fx = ReferenceFrame.mK.template at<float>(0, 0); mParams.fy = ReferenceFrame.mK.template at<float>(1, 1);
    mParams.cx = ReferenceFrame.mK.template at<float>(0, 2); mParams.cy = ReferenceFrame.mK.template at<float>(1, 2);
    mParams.sigma = sigma;
    mvKeys1 = ReferenceFrame.mvKeysUn;
  }

  // Computes in parallel a fundamental matrix and a homography; selects a model and tries to recover the motion and the structure
  bool Initialize(const FrameT& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                  std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
    const int n1 = (int)mvKeys1.size(), n2 = (int)CurrentFrame.mvKeysUn.size();
    if ((int)vMatches12.size() != n1) {
      fprintf(stderr, "orbfe_host::Initializer: %zu matches for %d keypoints of the reference frame\n", vMatches12.size(), n1);
      return false;
    }
    int N = 0;
    for (int i = 0; i < n1; i++) N += vMatches12[i] >= 0;
    if (N < 8) return false;
    // :76-93
    mvSets.assign((size_t)mMaxIterations * 8, 0);
    static bool seeded = false;   // DUtils::Random::SeedRandOnce(0)
    if (!seeded) {
      srand(0);
      seeded = true;
    }
    std::vector<int> vAvailableIndices;
    for (int it = 0; it < mMaxIterations; it++) {
      vAvailableIndices.resize(N);
      for (int i = 0; i < N; i++) vAvailableIndices[i] = i;
      for (size_t j = 0; j < 8; j++) {
        const int randi = RandomInt(0, (int)vAvailableIndices.size() - 1);
        mvSets[(size_t)it * 8 + j] = vAvailableIndices[randi];
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
    std::vector<float> k1((size_t)n1 * 2), k2((size_t)n2 * 2), p3d((size_t)n1 * 3);
    for (int i = 0; i < n1; i++) { k1[2 * i] = mvKeys1[i].pt.x; k1[2 * i + 1] = mvKeys1[i].pt.y; }
    for (int i = 0; i < n2; i++) { k2[2 * i] = CurrentFrame.mvKeysUn[i].pt.x; k2[2 * i + 1] = CurrentFrame.mvKeysUn[i].pt.y; }
    std::vector<int32_t> m12(vMatches12.begin(), vMatches12.end());
    const size_t nw = ((size_t)n1 + 63) / 64;
    std::vector<uint64_t> tri(nw), inl(nw);
    orbfe_init_params par = mParams;
    par.min_parallax = 1.0f;      // :115-119: ReconstructH / ReconstructF(..., 1.0, 50)
    par.min_triangulated = 50;
    const int rc = orbfe_initializer_initialize(&par, k1.data(), n1, k2.data(), n2, m12.data(), mvSets.data(), mMaxIterations, &mResult,
                                                p3d.data(), tri.data(), inl.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != ORBFE_OK) {
      fprintf(stderr, "orbfe_host::Initializer: orbfe_initializer_initialize failed (%d): %s\n", rc, orbfe_last_error());
      return false;
    }
    if (!mResult.success) return false;
    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R21.at<float>(r, c) = mResult.R21[3 * r + c];
      t21.at<float>(r, 0) = mResult.t21[r];
    }
    vP3D.resize(n1);
    vbTriangulated.assign(n1, false);
    for (int i = 0; i < n1; i++) {
      vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
      vbTriangulated[i] = (tri[i >> 6] >> (i & 63)) & 1;
    }
    return true;
  }

  // what decided the last Initialize(), and the sets it drew ([mMaxIterations][8])
  const orbfe_init_result& Result() const { return mResult; }
  const std::vector<int32_t>& Sets() const { return mvSets; }

 private:
  std::vector<cv::KeyPoint> mvKeys1;
  orbfe_init_params mParams;
  int mMaxIterations;
  std::vector<int32_t> mvSets;
  orbfe_init_result mResult = orbfe_init_result();
};

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
