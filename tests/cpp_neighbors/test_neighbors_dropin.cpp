// test_neighbors_dropin.cpp -- orbfe_host::SearchInNeighbors (csrc/host/LocalMapping_hip.h) on the mock KeyFrame / MapPoint of this
// directory, against the same function written with the per-keyframe ORBmatcher::Fuse (csrc/host/ORBmatcher.cc) on a second copy
// of the map.  usage: test_neighbors_dropin <scene.bin> <out.txt>; the scene is written by tests/test_neighbors_dropin_cpp.py, the
// output holds, for both runs, the return value and the whole map state (every keyframe's match table, every point's observations,
// flags, counters, descriptor, normal and distance range) as text.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/host/ORBmatcher.h"
#include "../../refactored_orb_slam2_amd/csrc/host/LocalMapping_hip.h"

using namespace ORB_SLAM2;

struct World {
  std::vector<KeyFrame> kfs;                        // one array: pointer order is index order
  std::vector<std::unique_ptr<MapPoint>> pts;
  int current = 0;
};

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static bool load(const char* path, World& w) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t hdr[4];   // n_kf, current, reserved, n_pts
  float cam[5], sf[ORBFE_MAX_LEVELS], inv[ORBFE_MAX_LEVELS], logsf;
  int32_t wh[2], n_levels;
  bool ok = rd(f, hdr, sizeof(hdr)) && rd(f, cam, sizeof(cam)) && rd(f, wh, sizeof(wh)) && rd(f, &n_levels, 4) && rd(f, &logsf, 4) &&
            rd(f, sf, sizeof(sf)) && rd(f, inv, sizeof(inv));
  if (!ok) return false;
  w.kfs.resize((size_t)hdr[0]);
  w.current = hdr[1];
  std::vector<std::vector<int32_t>> tables((size_t)hdr[0]), conn((size_t)hdr[0]);
  for (int k = 0; ok && k < hdr[0]; k++) {
    KeyFrame& K = w.kfs[(size_t)k];
    int32_t h[2];   // n, bad
    ok = rd(f, h, sizeof(h));
    K.N = h[0]; K.mbBad = h[1] != 0; K.mnId = (unsigned long)k + 1;
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mbf = cam[4]; K.invfx = 1.0f / K.fx; K.invfy = 1.0f / K.fy;
    K.mnMinX = 0; K.mnMaxX = wh[0]; K.mnMinY = 0; K.mnMaxY = wh[1];
    K.mnScaleLevels = n_levels; K.mfScaleFactor = sf[1]; K.mfLogScaleFactor = logsf;
    K.mvScaleFactors.assign(sf, sf + n_levels); K.mvInvLevelSigma2.assign(inv, inv + n_levels);
    for (int l = 0; l < n_levels; l++) K.mvLevelSigma2.push_back(sf[l] * sf[l]);
    K.Tcw = cv::Mat::eye(4, 4, CV_32F);
    K.Ow = cv::Mat::zeros(3, 1, CV_32F);
    K.mvKeysUn.resize((size_t)K.N); K.mvuRight.resize((size_t)K.N); K.mvDepth.assign((size_t)K.N, -1.f);
    K.mDescriptors = cv::Mat(K.N > 0 ? K.N : 1, 32, CV_8U);
    tables[(size_t)k].resize((size_t)K.N);
    ok = ok && rd(f, K.mvKeysUn.data(), sizeof(cv::KeyPoint) * (size_t)K.N) && rd(f, K.mDescriptors.ptr(0), (size_t)32 * K.N) &&
         rd(f, K.mvuRight.data(), 4 * (size_t)K.N) && rd(f, tables[(size_t)k].data(), 4 * (size_t)K.N);
    K.mvKeys = K.mvKeysUn;
    int32_t nc = 0;   // GetBestCovisibilityKeyFrames of this keyframe, best first
    ok = ok && rd(f, &nc, 4) && nc >= 0 && nc <= hdr[0];
    conn[(size_t)k].resize(ok ? (size_t)nc : 0);
    ok = ok && rd(f, conn[(size_t)k].data(), 4 * conn[(size_t)k].size());
  }
  for (int p = 0; ok && p < hdr[3]; p++) {
    float v[8];
    uint8_t d[32];
    int32_t h[2];   // bad, number of observations
    ok = rd(f, v, sizeof(v)) && rd(f, d, 32) && rd(f, h, sizeof(h));
    cv::Mat pos(3, 1, CV_32F), nrm(3, 1, CV_32F), desc(1, 32, CV_8U);
    for (int r = 0; r < 3; r++) { pos.at<float>(r) = v[r]; nrm.at<float>(r) = v[3 + r]; }
    memcpy(desc.ptr(0), d, 32);
    w.pts.emplace_back(new MapPoint(pos, nrm, desc, v[6], v[7]));
    MapPoint* P = w.pts.back().get();
    P->mnId = (unsigned long)p + 1;
    P->mbBad = h[0] != 0;
    for (int o = 0; ok && o < h[1]; o++) {
      int32_t e[2];
      ok = rd(f, e, sizeof(e));
      P->AddObservation(&w.kfs[(size_t)e[0]], (size_t)e[1]);
      if (!P->mpRefKF) P->mpRefKF = &w.kfs[(size_t)e[0]];
    }
  }
  fclose(f);
  if (!ok) return false;
  for (size_t k = 0; k < w.kfs.size(); k++)
    for (int32_t p : tables[k]) w.kfs[k].mvpMapPoints.push_back(p < 0 ? nullptr : w.pts[(size_t)p].get());
  for (size_t k = 0; k < w.kfs.size(); k++)
    for (int32_t c : conn[k]) w.kfs[k].mvpOrderedConnectedKeyFrames.push_back(&w.kfs[(size_t)c]);
  return true;
}

// LocalMapping::SearchInNeighbors as the reference writes it, on the drop-in ORBmatcher: one Fuse call per target keyframe
static int per_keyframe(KeyFrame* cur, bool bMonocular) {
  const std::vector<KeyFrame*> vpNeighKFs = cur->GetBestCovisibilityKeyFrames(bMonocular ? 20 : 10);
  std::vector<KeyFrame*> vpTargetKFs;
  for (KeyFrame* pKFi : vpNeighKFs) {
    if (pKFi->isBad() || pKFi->mnFuseTargetForKF == cur->mnId) continue;
    vpTargetKFs.push_back(pKFi);
    pKFi->mnFuseTargetForKF = cur->mnId;
    for (KeyFrame* pKFi2 : pKFi->GetBestCovisibilityKeyFrames(5)) {
      if (pKFi2->isBad() || pKFi2->mnFuseTargetForKF == cur->mnId || pKFi2->mnId == cur->mnId) continue;
      vpTargetKFs.push_back(pKFi2);
    }
  }
  ORBmatcher matcher(0.6f, true);
  int n = 0;
  std::vector<MapPoint*> vpMapPointMatches = cur->GetMapPointMatches();
  for (KeyFrame* pKFi : vpTargetKFs) n += matcher.Fuse(pKFi, vpMapPointMatches, 3.0f);
  std::vector<MapPoint*> cand;
  for (KeyFrame* pKFi : vpTargetKFs)
    for (MapPoint* pMP : pKFi->GetMapPointMatches()) {
      if (!pMP) continue;
      if (pMP->isBad() || pMP->mnFuseCandidateForKF == cur->mnId) continue;
      pMP->mnFuseCandidateForKF = cur->mnId;
      cand.push_back(pMP);
    }
  n += matcher.Fuse(cur, cand, 3.0f);
  if (orbfe_host::RefreshMapPoints(cur->GetMapPointMatches()) < 0) return -1;
  cur->UpdateConnections();
  return n;
}

static void dump(FILE* o, const char* name, int ret, World& w) {
  fprintf(o, "run %s ret %d connections %d\n", name, ret, w.kfs[(size_t)w.current].nUpdateConnections);
  fprintf(o, "state\n");
  for (size_t k = 0; k < w.kfs.size(); k++) {
    fprintf(o, "kf %zu mark %lu:", k, w.kfs[k].mnFuseTargetForKF);
    for (MapPoint* p : w.kfs[k].mvpMapPoints) fprintf(o, " %ld", p ? (long)p->mnId - 1 : -1L);
    fprintf(o, "\n");
  }
  for (size_t p = 0; p < w.pts.size(); p++) {
    MapPoint& P = *w.pts[p];
    fprintf(o, "pt %zu bad %d nobs %d found %d visible %d replaced %ld cand %lu obs", p, (int)P.mbBad, P.nObs, P.mnFound, P.mnVisible,
            P.mpReplaced ? (long)P.mpReplaced->mnId - 1 : -1L, P.mnFuseCandidateForKF);
    for (auto& kv : P.mObservations) fprintf(o, " %ld:%zu", (long)(kv.first - w.kfs.data()), kv.second);
    fprintf(o, " desc ");
    for (int i = 0; i < 32; i++) fprintf(o, "%02x", P.mDescriptor.ptr(0)[i]);
    fprintf(o, " geo %a %a %a %a %a\n", P.mNormalVector.at<float>(0), P.mNormalVector.at<float>(1), P.mNormalVector.at<float>(2), P.mfMinDistance,
            P.mfMaxDistance);
  }
  fprintf(o, "end\n");
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* o = fopen(argv[2], "w");
  if (!o) return 2;
  for (int mode = 0; mode < 2; mode++) {
    World w;
    if (!load(argv[1], w)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    KeyFrame* cur = &w.kfs[(size_t)w.current];
    const int ret = mode == 0 ? orbfe_host::SearchInNeighbors(cur, false) : per_keyframe(cur, false);
    dump(o, mode == 0 ? "batched" : "per_keyframe", ret, w);
  }
  fclose(o);
  return 0;
}
