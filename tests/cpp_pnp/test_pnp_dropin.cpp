// test_pnp_dropin.cpp -- orbfe_host::PnPsolver (csrc/host/PnPsolver_hip.h) on the mock Frame / MapPoint of this directory, in the loop
// shape of Tracking::Relocalization (L/src/Tracking.cc:1258-1363): one solver per candidate, SolveAll, then iterate(5) round robin
// until every candidate has reported bNoMore.
//   test_pnp_dropin <in.bin> <out.bin>
// in.bin  (written by tests/test_pnp_dropin_cpp.py): int32 S, uint32 seed of the generator, then S candidates, each float epsilon, 4
//         floats fx fy cx cy, int32 n_levels, n_levels float mvLevelSigma2, int32 n_slots, n_slots matches (int32 has_mp, bad, octave;
//         float Xw[3], u, v)
// out.bin: one record per iterate call: int32 candidate, int32 returned-a-matrix, 16 floats Tcw (zeros without), int32 nInliers, int32
//          bNoMore, int32 n_slots, n_slots bytes vbInliers; then per candidate int32 -1, N, mRansacMinInliers, mRansacMaxIts, status,
//          mnIterations, int32 number of sets, the sets, the N orbfe_pnp_point records
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "mock/Frame.h"
#include "../../refactored_orb_slam2_amd/csrc/host/PnPsolver_hip.h"

using namespace ORB_SLAM2;
typedef orbfe_host::PnPsolver<Frame, MapPoint> Solver;

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

struct Candidate {
  Frame frame;
  std::vector<std::unique_ptr<MapPoint>> owned;
  std::vector<MapPoint*> matches;
  std::unique_ptr<Solver> solver;
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t S = 0;
  uint32_t seed = 0;
  rd(f, &S, 1); rd(f, &seed, 1);
  uint64_t state = seed;   // one generator for all candidates, as the reference's rand() is
  auto below = [&state](int k) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (int)(((state >> 33) * (uint64_t)k) >> 31);
  };
  std::vector<std::unique_ptr<Candidate>> C;
  std::vector<Solver*> solvers;
  for (int k = 0; k < S; k++) {
    C.emplace_back(new Candidate());
    Candidate& c = *C.back();
    float eps = 0, cam[4];
    int32_t n_levels = 0, n_slots = 0;
    rd(f, &eps, 1); rd(f, cam, 4); rd(f, &n_levels, 1);
    c.frame.fx = cam[0]; c.frame.fy = cam[1]; c.frame.cx = cam[2]; c.frame.cy = cam[3];
    c.frame.mvLevelSigma2.resize(n_levels);
    rd(f, c.frame.mvLevelSigma2.data(), n_levels);
    rd(f, &n_slots, 1);
    c.frame.mvKeysUn.resize(n_slots);
    c.matches.assign(n_slots, nullptr);
    for (int i = 0; i < n_slots; i++) {
      int32_t m[3];
      float x[5];
      rd(f, m, 3); rd(f, x, 5);
      c.frame.mvKeysUn[i].pt.x = x[3]; c.frame.mvKeysUn[i].pt.y = x[4]; c.frame.mvKeysUn[i].octave = m[2];
      if (!m[0]) continue;
      c.owned.emplace_back(new MapPoint());
      MapPoint* p = c.owned.back().get();
      p->bad = m[1] != 0;
      p->pos = cv::Mat(3, 1, CV_32F);
      for (int r = 0; r < 3; r++) p->pos.at<float>(r) = x[r];
      c.matches[i] = p;
    }
    c.solver.reset(new Solver(c.frame, c.matches));
    c.solver->SetRansacParameters(0.99, 10, 300, 4, eps, 5.991);   // Tracking.cc:1262, epsilon from the case
    c.solver->SetRandom(below);
    solvers.push_back(c.solver.get());
  }
  fclose(f);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  Solver::SolveAll(solvers);
  std::vector<bool> discarded(S, false), vb;
  int left = S, nInliers = 0;
  while (left > 0) {   // :1290-1310 without the match that would end it early
    for (int k = 0; k < S; k++) {
      if (discarded[k]) continue;
      bool bNoMore = false;
      const cv::Mat T = solvers[k]->iterate(5, bNoMore, vb, nInliers);
      const int32_t head[2] = {k, !T.empty()};
      float t[16] = {0};
      if (!T.empty())
        for (int i = 0; i < 16; i++) t[i] = T.at<float>(i / 4, i % 4);
      const int32_t n_slots = (int32_t)C[k]->matches.size();
      std::vector<uint8_t> bytes(n_slots, 0);
      for (size_t i = 0; i < vb.size() && i < bytes.size(); i++) bytes[i] = vb[i] ? 1 : 0;
      const int32_t tail[3] = {nInliers, bNoMore, n_slots};
      wr(out, head, 2); wr(out, t, 16); wr(out, tail, 3); wr(out, bytes.data(), bytes.size());
      if (bNoMore) {
        discarded[k] = true;
        left--;
      }
    }
  }
  for (int k = 0; k < S; k++) {
    Solver& s = *solvers[k];
    const int32_t head[7] = {-1, s.NumCorrespondences(), s.MinInliers(), s.MaxIterations(), s.Status(), s.Iterations(), (int32_t)(s.Sets().size() / 4)};
    wr(out, head, 7);
    wr(out, s.Sets().data(), s.Sets().size());
    wr(out, s.Points().data(), s.Points().size());
  }
  fclose(out);
  return 0;
}
