// test_covis_dropin.cpp -- csrc/host/Covisibility_hip.h on the mock KeyFrame / MapPoint / Frame against the reference's loops restated
// on the same mocks in plain C++ (mock/MapPoint.h, and the two loops below), for tests/test_covis_dropin_cpp.py.
//   usage: test_covis_dropin check SEED     two identical seeded worlds; one goes through the adapter, the other through the plain
//                                           loops: UpdateConnections of every keyframe, the vote of every frame, KeyFrameCulling for
//                                           every third keyframe.  After each stage every member is compared: weights map, ordered
//                                           vectors, parent, children, bad flags, mbToBeErased, slots, observation maps, nObs, the
//                                           frames' vectors, the voted lists.  One line per stage; exit 0 when all are equal, 1 when
//                                           one differs, 3 when a library call failed (no device): that world is then as it was built.
//          test_covis_dropin bench OUT      times the plain loops alone on the three shapes of tools/bench_covis.py (one JSON line) and
//                                           writes the world they ran on to OUT
// The keyframes of a world live in one array, so the pointer order of every std::map<KeyFrame*, ...> is the order of their indices in
// both worlds; mnId is a permutation of the indices.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "mock/Frame.h"
#include "../../refactored_orb_slam2_amd/csrc/host/Covisibility_hip.h"

using ORB_SLAM2::Frame;
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  int below(int n) { return (int)(next() % (uint32_t)n); }
  float uniform(float a, float b) { return a + (b - a) * (float)(next() & 0xffffff) / 16777216.0f; }
};

struct World {
  std::vector<KeyFrame> kfs;
  std::vector<std::unique_ptr<MapPoint> > pts;
  std::vector<Frame> frames;
  std::vector<int> free_slot;
  World(int n_kf, int n_frames) : kfs((size_t)n_kf), frames((size_t)n_frames), free_slot((size_t)n_kf, 0) {}
};

// a map inside the stated domain: a slot holds a point exactly when the point holds that observation
static void build(World& W, uint64_t seed, int n_keys, int n_points, int window, int min_obs, int max_obs, int frame_slots) {
  Rng R(seed);
  const int n_kf = (int)W.kfs.size();
  for (int k = 0; k < n_kf; k++) {
    KeyFrame& K = W.kfs[k];
    K.mnId = (long unsigned int)((k * 7 + 3) % n_kf);   // a permutation for every n_kf that 7 does not divide
    K.mvKeysUn.resize((size_t)n_keys);
    K.mvuRight.assign((size_t)n_keys, -1.0f);
    K.mvDepth.assign((size_t)n_keys, -1.0f);
    K.mvpMapPoints.assign((size_t)n_keys, nullptr);
    K.mThDepth = 35.0f;
    K.mbNotErase = R.below(100) < 15;
  }
  for (int p = 0; p < n_points; p++) {
    const int c = R.below(n_kf), n_want = min_obs + R.below(max_obs - min_obs + 1), base = R.below(5);
    std::vector<int> near;
    for (int k = c - window < 0 ? 0 : c - window; k <= c + window && k < n_kf; k++)
      if (W.free_slot[k] < n_keys) near.push_back(k);
    if ((int)near.size() < 2) continue;
    std::unique_ptr<MapPoint> M(new MapPoint);
    for (int j = 0; j < n_want && !near.empty(); j++) {
      const int at = R.below((int)near.size()), k = near[at];
      near.erase(near.begin() + at);
      KeyFrame& K = W.kfs[k];
      const int i = W.free_slot[k]++;
      K.mvKeysUn[i].octave = base + R.below(2);
      K.mvuRight[i] = R.below(2) ? 10.0f : -1.0f;
      K.mvDepth[i] = R.uniform(0.0f, 38.0f);
      K.mvpMapPoints[i] = M.get();
      M->AddObservation(&K, (size_t)i);
      if (!M->mpRefKF) M->mpRefKF = &K;
    }
    W.pts.push_back(std::move(M));
  }
  const size_t n_good = W.pts.size();
  for (int b = 0; b < 10; b++) {   // bad points: no observations, in no keyframe, but still in a frame's vector
    std::unique_ptr<MapPoint> M(new MapPoint);
    M->mbBad = true;
    W.pts.push_back(std::move(M));
  }
  for (size_t f = 0; f < W.frames.size(); f++) {
    Frame& F = W.frames[f];
    F.mnId = 100 + f;
    F.N = frame_slots;
    F.mvpMapPoints.assign((size_t)frame_slots, nullptr);
    const int c = R.below(n_kf);
    for (int i = 0; i < frame_slots; i++) {
      const int roll = R.below(10);
      if (roll < 3) continue;
      if (roll == 3) { F.mvpMapPoints[i] = W.pts[n_good + (size_t)R.below(10)].get(); continue; }
      // a point seen near keyframe c, so that frames vote for neighbourhoods
      const KeyFrame& K = W.kfs[(c + R.below(3)) % n_kf];
      F.mvpMapPoints[i] = K.mvpMapPoints[(size_t)R.below(n_keys)];
    }
  }
}

// Tracking.cc:1117-1159 on the mocks: 1, or 0 for the early return
static int plain_vote(Frame& F, std::vector<KeyFrame*>& vpLocalKeyFrames, KeyFrame*& pKFmax) {
  std::map<KeyFrame*, int> keyframeCounter;
  for (int i = 0; i < F.N; i++) {
    MapPoint* pMP = F.mvpMapPoints[i];
    if (!pMP) continue;
    if (pMP->isBad()) { F.mvpMapPoints[i] = nullptr; continue; }
    const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
    for (std::map<KeyFrame*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) keyframeCounter[it->first]++;
  }
  if (keyframeCounter.empty()) return 0;
  int max = 0;
  pKFmax = nullptr;
  vpLocalKeyFrames.clear();
  for (std::map<KeyFrame*, int>::const_iterator it = keyframeCounter.begin(); it != keyframeCounter.end(); ++it) {
    KeyFrame* pKF = it->first;
    if (pKF->isBad()) continue;
    if (it->second > max) { max = it->second; pKFmax = pKF; }
    vpLocalKeyFrames.push_back(pKF);
    pKF->mnTrackReferenceForFrame = F.mnId;
  }
  return 1;
}

// LocalMapping.cc:595-655 on the mocks; returns the number of SetBadFlag() calls
static int plain_culling(KeyFrame* pCurrentKF, bool bMonocular) {
  const std::vector<KeyFrame*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
  int n = 0;
  for (size_t j = 0; j < vpLocalKeyFrames.size(); j++) {
    KeyFrame* pKF = vpLocalKeyFrames[j];
    if (pKF->mnId == 0) continue;
    const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
    const int thObs = 3;
    int nRedundantObservations = 0, nMPs = 0;
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
      MapPoint* pMP = vpMapPoints[i];
      if (!pMP || pMP->isBad()) continue;
      if (!bMonocular && (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0)) continue;
      nMPs++;
      if (pMP->Observations() <= thObs) continue;
      const int scaleLevel = pKF->mvKeysUn[i].octave;
      const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
      int nObs = 0;
      for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit) {
        KeyFrame* pKFi = mit->first;
        if (pKFi == pKF) continue;
        if (pKFi->mvKeysUn[mit->second].octave <= scaleLevel + 1 && ++nObs >= thObs) break;
      }
      if (nObs >= thObs) nRedundantObservations++;
    }
    if (nRedundantObservations > 0.9 * nMPs) {
      pKF->SetBadFlag();
      n++;
    }
  }
  return n;
}

// every member the three functions touch, by index
static std::string dump(World& W) {
  std::map<const KeyFrame*, int> ki;
  std::map<const MapPoint*, int> pi;
  for (size_t k = 0; k < W.kfs.size(); k++) ki[&W.kfs[k]] = (int)k;
  for (size_t p = 0; p < W.pts.size(); p++) pi[W.pts[p].get()] = (int)p;
  std::ostringstream o;
  for (size_t k = 0; k < W.kfs.size(); k++) {
    KeyFrame& K = W.kfs[k];
    o << "K" << k << " bad" << K.mbBad << " tbe" << K.mbToBeErased << " first" << K.mbFirstConnection << " ref" << K.mnTrackReferenceForFrame
      << " parent" << (K.mpParent ? ki[K.mpParent] : -1) << " w{";
    for (std::map<KeyFrame*, int>::iterator it = K.mConnectedKeyFrameWeights.begin(); it != K.mConnectedKeyFrameWeights.end(); ++it)
      o << ki[it->first] << ":" << it->second << ",";
    o << "} o[";
    for (size_t i = 0; i < K.mvpOrderedConnectedKeyFrames.size(); i++) o << ki[K.mvpOrderedConnectedKeyFrames[i]] << ",";
    o << "] ow[";
    for (size_t i = 0; i < K.mvOrderedWeights.size(); i++) o << K.mvOrderedWeights[i] << ",";
    o << "] c{";
    for (std::set<KeyFrame*>::iterator it = K.mspChildrens.begin(); it != K.mspChildrens.end(); ++it) o << ki[*it] << ",";
    o << "} s[";
    for (size_t i = 0; i < K.mvpMapPoints.size(); i++) o << (K.mvpMapPoints[i] ? pi[K.mvpMapPoints[i]] : -1) << ",";
    o << "]\n";
  }
  for (size_t p = 0; p < W.pts.size(); p++) {
    MapPoint& M = *W.pts[p];
    o << "P" << p << " bad" << M.mbBad << " n" << M.nObs << " ref" << (M.mpRefKF ? ki[M.mpRefKF] : -1) << " {";
    for (std::map<KeyFrame*, size_t>::iterator it = M.mObservations.begin(); it != M.mObservations.end(); ++it) o << ki[it->first] << ":" << it->second << ",";
    o << "}\n";
  }
  for (size_t f = 0; f < W.frames.size(); f++) {
    o << "F" << f << " [";
    for (size_t i = 0; i < W.frames[f].mvpMapPoints.size(); i++) o << (W.frames[f].mvpMapPoints[i] ? pi[W.frames[f].mvpMapPoints[i]] : -1) << ",";
    o << "]\n";
  }
  return o.str();
}

static bool stage(const char* name, World& A, World& B, const std::string& extraA, const std::string& extraB, int count) {
  const bool equal = dump(A) == dump(B) && extraA == extraB;
  printf("%s %s %d\n", name, equal ? "EQUAL" : "DIFFERENT", count);
  return equal;
}

static int check(uint64_t seed) {
  const int n_kf = 20, n_frames = 6;
  World A(n_kf, n_frames), B(n_kf, n_frames);
  build(A, seed, 150, 380, 3, 4, 7, 120);
  build(B, seed, 150, 380, 3, 4, 7, 120);
  if (dump(A) != dump(B)) return 2;
  bool failed = false, equal = true;
  // 1. UpdateConnections of every keyframe, in array order reversed so that the list order is not the pointer order
  std::vector<KeyFrame*> vpKFs;
  for (int k = n_kf - 1; k >= 0; k--) vpKFs.push_back(&A.kfs[k]);
  const int updated = ORB_SLAM2::orbfe_host::UpdateConnectionsBatch(vpKFs);
  failed = failed || updated < 0;
  for (int k = n_kf - 1; k >= 0; k--) B.kfs[k].UpdateConnections();
  equal = stage("connections", A, B, "", "", updated) && equal;
  // 2. the vote of every frame
  std::ostringstream va, vb;
  int voted = 0;
  for (int f = 0; f < n_frames; f++) {
    std::vector<KeyFrame*> la, lb;
    KeyFrame *ma = nullptr, *mb = nullptr;
    const int ra = ORB_SLAM2::orbfe_host::VoteLocalKeyFrames(A.frames[f], la, ma), rb = plain_vote(B.frames[f], lb, mb);
    failed = failed || ra < 0;
    voted += ra > 0;
    va << ra << " max" << (ma ? (int)(ma - &A.kfs[0]) : -1) << " [";
    vb << rb << " max" << (mb ? (int)(mb - &B.kfs[0]) : -1) << " [";
    for (size_t i = 0; i < la.size(); i++) va << (int)(la[i] - &A.kfs[0]) << ",";
    for (size_t i = 0; i < lb.size(); i++) vb << (int)(lb[i] - &B.kfs[0]) << ",";
  }
  equal = stage("votes", A, B, va.str(), vb.str(), voted) && equal;
  // 3. KeyFrameCulling for every third keyframe that is still alive, alternating the sensor kind
  int culled_a = 0, culled_b = 0;
  for (int k = 1; k < n_kf; k += 3) {
    if (B.kfs[k].isBad()) continue;
    const int ra = ORB_SLAM2::orbfe_host::KeyFrameCulling(&A.kfs[k], (k & 1) != 0);
    failed = failed || ra < 0;
    culled_a += ra > 0 ? ra : 0;
    culled_b += plain_culling(&B.kfs[k], (k & 1) != 0);
    std::ostringstream name;
    name << "culling" << k;
    equal = stage(name.str().c_str(), A, B, "", "", culled_a) && equal;
  }
  printf("set_bad_flag_calls %d %d\n", culled_a, culled_b);
  if (failed) return 3;
  return equal && culled_a == culled_b ? 0 : 1;
}

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static void put(FILE* f, const void* p, size_t bytes) { if (bytes) fwrite(p, 1, bytes, f); }

// The plain loops alone (no library call), -O2, on the shapes of tools/bench_covis.py, and the world they ran on written to `path` so
// that the device runs on the same map: int32 n_kf, n_keys, n_points, n_frames, frame_slots, subject, n_local, local[n_local]; per
// keyframe int32 flags (1: mnId == 0, 2: mbNotErase), float mThDepth, int32 octave[n_keys], float mvuRight[n_keys], float
// mvDepth[n_keys], int32 slot[n_keys]; per point int32 bad, nObs, n, {kf, idx}[n] in map order; int32 frame slot[n_frames][frame_slots].
// No keyframe gets a spanning-tree parent here (mbFirstConnection is cleared): the tree is not part of what is timed.
static int bench(const char* path) {
  const int n_kf = 60, n_keys = 2000, n_frames = 256, frame_slots = 2000, subject = 30;
  World W(n_kf, n_frames);
  build(W, 1, n_keys, 14000, 20, 6, 10, frame_slots);
  for (KeyFrame& K : W.kfs) K.mbFirstConnection = false;
  FILE* f = fopen(path, "wb");
  if (!f) return 2;
  std::map<const MapPoint*, int32_t> pi;
  for (size_t p = 0; p < W.pts.size(); p++) pi[W.pts[p].get()] = (int32_t)p;
  // 1. one keyframe of 2 000 slots at about 8 observations per point
  double conn[2], votes[2], cull[2];
  for (int r = 0; r < 2; r++) {
    const double t0 = now_ms();
    W.kfs[subject].UpdateConnections();
    conn[r] = now_ms() - t0;
  }
  // what the loop left on the subject, for the device's header to be compared with: weights, ordered entries, pKFmax by row, nmax
  KeyFrame& Sj = W.kfs[subject];
  int conn_check[4] = {(int)Sj.mConnectedKeyFrameWeights.size(), (int)Sj.mvOrderedWeights.size(), -1, 0};
  for (std::map<KeyFrame*, int>::iterator it = Sj.mConnectedKeyFrameWeights.begin(); it != Sj.mConnectedKeyFrameWeights.end(); ++it)
    if (it->second > conn_check[3]) { conn_check[3] = it->second; conn_check[2] = (int)(it->first - &W.kfs[0]); }
  long long ordered_sum = 0;   // position-weighted, so that the order of the list counts
  for (size_t i = 0; i < Sj.mvpOrderedConnectedKeyFrames.size(); i++) ordered_sum += (long long)(i + 1) * (Sj.mvpOrderedConnectedKeyFrames[i] - &W.kfs[0]);
  // 2. 256 frames
  std::vector<int32_t> frame_slot;
  for (Frame& F : W.frames)
    for (MapPoint* pMP : F.mvpMapPoints) frame_slot.push_back(pMP ? pi[pMP] : -1);
  long long vote_check[3] = {0, 0, 0};   // over the frames: voted keyframes, position-weighted rows of the lists, rows of pKFmax
  for (int r = 0; r < 2; r++) {
    vote_check[0] = vote_check[1] = vote_check[2] = 0;
    const double t0 = now_ms();
    for (Frame& F : W.frames) {
      std::vector<KeyFrame*> local;
      KeyFrame* mx = nullptr;
      plain_vote(F, local, mx);
      vote_check[0] += (long long)local.size();
      for (size_t i = 0; i < local.size(); i++) vote_check[1] += (long long)(i + 1) * (local[i] - &W.kfs[0]);
      vote_check[2] += mx ? (long long)(mx - &W.kfs[0]) : -1;
    }
    votes[r] = now_ms() - t0;
  }
  // 3. one culling problem with 40 local keyframes; it mutates the map, so each run has a world of its own
  std::vector<int32_t> local;
  int n_set_bad = 0;
  for (int r = 0; r < 2; r++) {
    World C(n_kf, 1);
    build(C, 1, n_keys, 14000, 20, 6, 10, 8);
    for (KeyFrame& K : C.kfs) K.mbFirstConnection = false;
    for (KeyFrame& K : C.kfs) K.UpdateConnections();
    KeyFrame* cur = &C.kfs[subject];
    if (cur->mvpOrderedConnectedKeyFrames.size() > 40) cur->mvpOrderedConnectedKeyFrames.resize(40);
    local.clear();
    for (KeyFrame* pKF : cur->mvpOrderedConnectedKeyFrames) local.push_back((int32_t)(pKF - &C.kfs[0]));
    const double t0 = now_ms();
    n_set_bad = plain_culling(cur, false);
    cull[r] = now_ms() - t0;
  }
  const int32_t head[7] = {n_kf, n_keys, (int32_t)W.pts.size(), n_frames, frame_slots, subject, (int32_t)local.size()};
  put(f, head, sizeof(head));
  put(f, local.data(), local.size() * 4);
  for (KeyFrame& K : W.kfs) {
    const int32_t flags = (K.mnId == 0 ? 1 : 0) | (K.mbNotErase ? 2 : 0);
    put(f, &flags, 4);
    put(f, &K.mThDepth, 4);
    std::vector<int32_t> oct, slot;
    for (int i = 0; i < n_keys; i++) {
      oct.push_back(K.mvKeysUn[i].octave);
      slot.push_back(K.mvpMapPoints[i] ? pi[K.mvpMapPoints[i]] : -1);
    }
    put(f, oct.data(), oct.size() * 4);
    put(f, K.mvuRight.data(), K.mvuRight.size() * 4);
    put(f, K.mvDepth.data(), K.mvDepth.size() * 4);
    put(f, slot.data(), slot.size() * 4);
  }
  for (size_t p = 0; p < W.pts.size(); p++) {
    MapPoint& M = *W.pts[p];
    const int32_t h[3] = {M.mbBad ? 1 : 0, M.nObs, (int32_t)M.mObservations.size()};
    put(f, h, sizeof(h));
    for (std::map<KeyFrame*, size_t>::iterator it = M.mObservations.begin(); it != M.mObservations.end(); ++it) {
      const int32_t o[2] = {(int32_t)(it->first - &W.kfs[0]), (int32_t)it->second};
      put(f, o, sizeof(o));
    }
  }
  put(f, frame_slot.data(), frame_slot.size() * 4);
  fclose(f);
  printf("{\"connections_ms\": [%.4f, %.4f], \"votes_256_ms\": [%.4f, %.4f], \"culling_ms\": [%.4f, %.4f], \"culling_local\": %d, "
         "\"culling_set_bad\": %d, \"conn_check\": [%d, %d, %d, %d, %lld], \"vote_check\": [%lld, %lld, %lld]}\n", conn[0], conn[1], votes[0], votes[1],
         cull[0], cull[1], (int)local.size(), n_set_bad, conn_check[0], conn_check[1], conn_check[2], conn_check[3], ordered_sum,
         vote_check[0], vote_check[1], vote_check[2]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "bench")) return bench(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "check")) return check((uint64_t)atoll(argv[2]));
  return 2;
}
