// test_egraph_dropin.cpp -- orbfe_host::OptimizeEssentialGraph (csrc/host/Optimizer_hip.h) and orbfe_host::CorrectLoopPropagate
// (csrc/host/LoopClosing_hip.h) on the mock Sim3 / KeyFrame / MapPoint / Map of mock_egraph/Types.h.
//   test_egraph_dropin <in.bin> <out.bin> marshal | run | propagate
// in.bin (written by tests/test_egraph_dropin_cpp.py), int32 and float / double fields:
//   int32 fix_scale, NK; per keyframe: int32 mnId, bad; 12 floats [R | t]; int32 parent index (-1: none); int32 n + n keyframe indices
//   (GetLoopEdges); int32 n + n x (int32 keyframe index, int32 weight); int32 has + 8 doubles (CorrectedSim3 entry); the same for
//   NonCorrectedSim3; then int32 loop keyframe index, current keyframe index; int32 n + n x (int32 keyframe index, int32 m + m indices)
//   (LoopConnections); int32 NM; per point: int32 mnId, bad; 3 floats; int32 reference keyframe index, mnCorrectedByKF,
//   mnCorrectedReference; int32 n + n keyframe indices that observe it (keypoint 0 of each); for `propagate`: int32 n + n keyframe
//   indices (mvpCurrentConnectedKFs) and 8 doubles (mg2oScw).
// out.bin: `marshal`: int32 n_kf + mnIds, the vertex records, int32 n_edges + the edge records, int32 n_points + ref + 3 floats each.
//   `run` (needs a device): per keyframe int32 SetPose calls + 12 floats; per point int32 SetWorldPos calls + 3 floats + min / max
//   distance + 3 floats of the normal.  `propagate` (needs a device): int32 return value; int32 n + n x (int32 mnId, 8 doubles) of
//   CorrectedSim3 and of NonCorrectedSim3, both ascending by mnId; then as `run`, with int32 mnCorrectedByKF, mnCorrectedReference behind
//   each point.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "mock_egraph/Types.h"
#include "../../refactored_orb_slam2_amd/csrc/host/LoopClosing_hip.h"

using namespace ORB_SLAM2;
typedef std::map<KeyFrame*, mockg2o::Sim3> KeyFrameAndPose;

static std::vector<uint8_t> raw;
static size_t off = 0;
template <class T>
static T get() {
  T v;
  if (off + sizeof(T) > raw.size()) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  memcpy(&v, raw.data() + off, sizeof(T));
  off += sizeof(T);
  return v;
}
static mockg2o::Sim3 get_sim3() {
  mockg2o::Sim3 S;
  S.r.qx = get<double>(); S.r.qy = get<double>(); S.r.qz = get<double>(); S.r.qw = get<double>();
  for (int k = 0; k < 3; k++) S.t[k] = get<double>();
  S.s = get<double>();
  return S;
}
template <class T>
static void wr(FILE* f, const T* p, size_t n) {
  if (n) fwrite(p, sizeof(T), n, f);
}
static void wr32(FILE* f, long v) {
  const int32_t x = (int32_t)v;
  wr(f, &x, 1);
}
static void wr_sim3(FILE* f, const mockg2o::Sim3& S) {
  const orbfe_eg_sim3 r = orbfe_host::EssentialGraphRecord(S);
  wr(f, &r, 1);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  fseek(fi, 0, SEEK_END);
  raw.resize((size_t)ftell(fi));
  fseek(fi, 0, SEEK_SET);
  if (fread(raw.data(), 1, raw.size(), fi) != raw.size()) return 2;
  fclose(fi);
  const std::string mode = argv[3];

  const bool fix_scale = get<int32_t>() != 0;
  const int NK = get<int32_t>();
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  for (int k = 0; k < NK; k++) kfs.emplace_back(new KeyFrame());
  KeyFrameAndPose Corrected, NonCorrected;
  Map map;
  for (int k = 0; k < NK; k++) {
    KeyFrame& K = *kfs[k];
    K.mnId = (long unsigned int)get<int32_t>();
    K.bad = get<int32_t>() != 0;
    K.Tcw = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) K.Tcw.at<float>(r, c) = get<float>();
    const int parent = get<int32_t>();
    if (parent >= 0) {
      K.parent = kfs[parent].get();
      kfs[parent]->children.insert(&K);
    }
    for (int n = get<int32_t>(); n > 0; n--) K.loop_edges.insert(kfs[get<int32_t>()].get());
    for (int n = get<int32_t>(); n > 0; n--) {
      const int j = get<int32_t>();
      K.weights[kfs[j].get()] = get<int32_t>();
    }
    if (get<int32_t>()) Corrected[&K] = get_sim3();
    if (get<int32_t>()) NonCorrected[&K] = get_sim3();
    K.mnScaleLevels = 8;
    for (int l = 0; l < 8; l++) K.mvScaleFactors.push_back(l == 0 ? 1.0f : K.mvScaleFactors[l - 1] * 1.2f);
    K.mvKeysUn.resize(1);
    K.mvKeysUn[0].octave = k % 3;
    K.mDescriptors = cv::Mat::zeros(1, 32, CV_8U);
    map.keyframes.push_back(&K);
  }
  std::reverse(map.keyframes.begin(), map.keyframes.end());   // GetAllKeyFrames() promises no order
  KeyFrame* pLoopKF = kfs[get<int32_t>()].get();
  KeyFrame* pCurKF = kfs[get<int32_t>()].get();
  std::map<KeyFrame*, std::set<KeyFrame*>> LoopConnections;
  for (int n = get<int32_t>(); n > 0; n--) {
    KeyFrame* a = kfs[get<int32_t>()].get();
    for (int m = get<int32_t>(); m > 0; m--) LoopConnections[a].insert(kfs[get<int32_t>()].get());
  }
  const int NM = get<int32_t>();
  std::vector<std::unique_ptr<MapPoint>> mps;
  for (int p = 0; p < NM; p++) {
    mps.emplace_back(new MapPoint());
    MapPoint& M = *mps.back();
    M.mnId = (long unsigned int)get<int32_t>();
    M.bad = get<int32_t>() != 0;
    M.pos = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) M.pos.at<float>(r) = get<float>();
    M.mpRefKF = kfs[get<int32_t>()].get();
    M.mnCorrectedByKF = (long unsigned int)get<int32_t>();
    M.mnCorrectedReference = (long unsigned int)get<int32_t>();
    for (int n = get<int32_t>(); n > 0; n--) {
      KeyFrame* K = kfs[get<int32_t>()].get();
      M.observations[K] = 0;
      K->mvpMapPoints.push_back(&M);
    }
    M.mNormalVector = cv::Mat::zeros(3, 1, CV_32F);
    map.points.push_back(&M);
  }

  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  auto dump_state = [&](bool marks) {
    for (int k = 0; k < NK; k++) {
      wr32(fo, kfs[k]->set_pose_calls);
      for (int r = 0; r < 3; r++) wr(fo, kfs[k]->Tcw.ptr<float>(r), 4);
    }
    for (int p = 0; p < NM; p++) {
      wr32(fo, mps[p]->set_pos_calls);
      for (int r = 0; r < 3; r++) wr(fo, &mps[p]->pos.at<float>(r), 1);
      wr(fo, &mps[p]->mfMinDistance, 1);
      wr(fo, &mps[p]->mfMaxDistance, 1);
      for (int r = 0; r < 3; r++) wr(fo, &mps[p]->mNormalVector.at<float>(r), 1);
      if (marks) {
        wr32(fo, (long)mps[p]->mnCorrectedByKF);
        wr32(fo, (long)mps[p]->mnCorrectedReference);
      }
    }
  };
  if (mode == "marshal") {
    orbfe_host::EssentialGraphProblem<KeyFrame, MapPoint> B;
    orbfe_host::OptimizeEssentialGraphMarshal(&map, pLoopKF, pCurKF, NonCorrected, Corrected, LoopConnections, B);
    wr32(fo, (long)B.vpKFs.size());
    for (KeyFrame* K : B.vpKFs) wr32(fo, (long)K->mnId);
    wr(fo, B.vertices.data(), B.vertices.size());
    wr32(fo, (long)B.edges.size());
    wr(fo, B.edges.data(), B.edges.size());
    wr32(fo, (long)B.vpMPs.size());
    wr(fo, B.ref.data(), B.ref.size());
    wr(fo, B.points.data(), B.points.size());
  } else if (mode == "run") {
    orbfe_host::OptimizeEssentialGraph(&map, pLoopKF, pCurKF, NonCorrected, Corrected, LoopConnections, fix_scale);
    dump_state(false);
  } else if (mode == "propagate") {
    std::vector<KeyFrame*> connected;
    for (int n = get<int32_t>(); n > 0; n--) connected.push_back(kfs[get<int32_t>()].get());
    const mockg2o::Sim3 Scw = get_sim3();
    KeyFrameAndPose C2, N2;
    wr32(fo, orbfe_host::CorrectLoopPropagate(pCurKF, connected, Scw, C2, N2));
    for (KeyFrameAndPose* M : {&C2, &N2}) {
      std::vector<std::pair<long, const mockg2o::Sim3*>> v;
      for (const auto& p : *M) v.push_back(std::make_pair((long)p.first->mnId, &p.second));
      std::sort(v.begin(), v.end());
      wr32(fo, (long)v.size());
      for (const auto& p : v) {
        wr32(fo, p.first);
        wr_sim3(fo, *p.second);
      }
    }
    dump_state(true);
  } else {
    return 2;
  }
  fclose(fo);
  return 0;
}
