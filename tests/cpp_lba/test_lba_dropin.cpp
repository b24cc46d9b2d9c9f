// test_lba_dropin.cpp -- orbfe_host::LocalBundleAdjustment (csrc/host/Optimizer_hip.h) on the mock KeyFrame / MapPoint / Map of this
// directory.
//   test_lba_dropin <in.bin> <out.bin> run | apply
// in.bin  (written by tests/test_lba_dropin_cpp.py): int32 S, then S scenes, each
//         int32 stop_flag; 5 floats fx fy cx cy mbf; int32 n_levels, n_levels float mvInvLevelSigma2;
//         int32 NK, NK keyframes (int32 mnId, int32 bad, 12 floats of [R | t], int32 n_kp, n_kp x (float x, float y, int32 octave,
//         float mvuRight)); int32 index of pKF; int32 n_cov, n_cov int32 keyframe indices (GetVectorCovisibleKeyFrames);
//         int32 NM, NM map points (int32 mnId, int32 bad, 3 floats, int32 n_obs, n_obs x (int32 keyframe index, int32 keypoint));
//         for `apply` a synthetic result follows: int32 n_erase, n_erase x (int32 keyframe mnId, int32 point mnId), a float added to
//         every pose entry and a float added to every point coordinate
// out.bin per scene: the marshalled problem of a first copy of the scene (int32 n_local + mnIds, int32 n_fixed + mnIds, int32 n_mp +
//         mnIds, int32 n_kf + fixed bytes + n_kf x 12 floats, int32 n_points x 3 floats, int32 n_edges x (orbfe_lba_edge, int32
//         keyframe mnId, int32 point mnId)) and its marks (NK x (int32 mnBALocalForKF, mnBAFixedForKF), NM x int32 mnBALocalForKF);
//         then, of a second copy after the call (`run`: LocalBundleAdjustment, `apply`: marshal + the synthetic result applied):
//         NK x (int32 SetPose calls, 12 floats), NM x (int32 SetWorldPos calls, int32 UpdateNormalAndDepth calls, 3 floats), int32
//         count + pairs (keyframe mnId, point mnId) of EraseMapPointMatch, the same of EraseObservation, NK x NM bytes "keyframe
//         still matches the point" and NM x NK bytes "point still observes the keyframe"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "mock/KeyFrame.h"
#include "mock/Map.h"
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
static void wr32(FILE* f, long v) {
  const int32_t x = (int32_t)v;
  wr(f, &x, 1);
}

struct Scene {
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<MapPoint>> mps;
  KeyFrame* pKF = nullptr;
  bool stop = false;
};

static void build(const std::vector<uint8_t>& raw, size_t& off, Scene& S) {
  auto get = [&raw, &off](void* p, size_t n) {
    if (off + n > raw.size()) {
      fprintf(stderr, "short input\n");
      exit(2);
    }
    memcpy(p, raw.data() + off, n);
    off += n;
  };
  int32_t stop = 0, n_levels = 0, NK = 0, NM = 0, cur = 0, n_cov = 0;
  float cam[5];
  get(&stop, 4);
  get(cam, 20);
  get(&n_levels, 4);
  std::vector<float> sig(n_levels);
  get(sig.data(), 4 * (size_t)n_levels);
  S.stop = stop != 0;
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
    K.mvKeysUn.resize(n_kp);
    K.mvuRight.resize(n_kp);
    K.mvpMapPoints.assign(n_kp, nullptr);
    for (int i = 0; i < n_kp; i++) {
      float xy[2], ur;
      int32_t oct;
      get(xy, 8);
      get(&oct, 4);
      get(&ur, 4);
      K.mvKeysUn[i].pt.x = xy[0];
      K.mvKeysUn[i].pt.y = xy[1];
      K.mvKeysUn[i].octave = oct;
      K.mvuRight[i] = ur;
    }
  }
  get(&cur, 4);
  S.pKF = S.kfs[cur].get();
  get(&n_cov, 4);
  for (int i = 0; i < n_cov; i++) {
    int32_t k = 0;
    get(&k, 4);
    S.pKF->covisible.push_back(S.kfs[k].get());
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
      int32_t ko[2];
      get(ko, 8);
      M.observations[S.kfs[ko[0]].get()] = (size_t)ko[1];
      S.kfs[ko[0]]->mvpMapPoints[ko[1]] = &M;
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const bool apply = strcmp(argv[3], "apply") == 0;
  FILE* f = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!f || !out) return 2;
  std::vector<uint8_t> raw;
  {
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + n);
  }
  fclose(f);
  size_t off = 0;
  int32_t S = 0;
  memcpy(&S, raw.data(), 4);
  off = 4;
  for (int s = 0; s < S; s++) {
    const size_t begin = off;
    Scene one, two;
    build(raw, off, one);
    size_t again = begin;
    build(raw, again, two);
    {   // what the adapter collects and marshals, and the marks it leaves
      orbfe_host::LocalBAProblem<KeyFrame, MapPoint> B;
      orbfe_host::LocalBundleAdjustmentMarshal(one.pKF, B);
      wr32(out, (long)B.lLocalKeyFrames.size());
      for (KeyFrame* k : B.lLocalKeyFrames) wr32(out, (long)k->mnId);
      wr32(out, (long)B.lFixedCameras.size());
      for (KeyFrame* k : B.lFixedCameras) wr32(out, (long)k->mnId);
      wr32(out, (long)B.lLocalMapPoints.size());
      for (MapPoint* m : B.lLocalMapPoints) wr32(out, (long)m->mnId);
      wr32(out, (long)B.fixed.size());
      wr(out, B.fixed.data(), B.fixed.size());
      wr(out, B.poses.data(), B.poses.size());
      wr32(out, (long)(B.points.size() / 3));
      wr(out, B.points.data(), B.points.size());
      wr32(out, (long)B.edges.size());
      for (size_t i = 0; i < B.edges.size(); i++) {
        wr(out, &B.edges[i], 1);
        wr32(out, (long)B.vpEdgeKF[i]->mnId);
        wr32(out, (long)B.vpMapPointEdge[i]->mnId);
      }
      for (auto& k : one.kfs) {
        wr32(out, (long)k->mnBALocalForKF);
        wr32(out, (long)k->mnBAFixedForKF);
      }
      for (auto& m : one.mps) wr32(out, (long)m->mnBALocalForKF);
    }
    Map map;
    if (apply) {
      int32_t n_erase = 0;
      memcpy(&n_erase, raw.data() + off, 4);
      off += 4;
      std::vector<int32_t> pairs(2 * (size_t)n_erase);
      memcpy(pairs.data(), raw.data() + off, 8 * (size_t)n_erase);
      off += 8 * (size_t)n_erase;
      float add[2];
      memcpy(add, raw.data() + off, 8);
      off += 8;
      orbfe_host::LocalBAProblem<KeyFrame, MapPoint> B;
      orbfe_host::LocalBundleAdjustmentMarshal(two.pKF, B);
      std::vector<float> po(B.poses), xo(B.points);
      for (float& v : po) v += add[0];
      for (float& v : xo) v += add[1];
      std::vector<uint8_t> erase(B.edges.size(), 0);
      for (size_t i = 0; i < B.edges.size(); i++)
        for (int e = 0; e < n_erase; e++)
          if ((long)B.vpEdgeKF[i]->mnId == pairs[2 * e] && (long)B.vpMapPointEdge[i]->mnId == pairs[2 * e + 1])
            erase[i] = ORBFE_LBA_ERASE | ORBFE_LBA_DROPPED;
      for (size_t i = 0; i < B.edges.size(); i++)
        if (!erase[i] && (i % 3) == 0) erase[i] = ORBFE_LBA_DROPPED;   // dropped in round 1 alone is not on the erase list
      if (!two.stop) orbfe_host::LocalBundleAdjustmentApply(B, po.data(), xo.data(), erase.data(), &map);
    } else {
      bool stop = two.stop;
      orbfe_host::LocalBundleAdjustment(two.pKF, &stop, &map);
    }
    if (!map.mMutexMapUpdate.try_lock()) return 3;   // the adapter must have released it
    map.mMutexMapUpdate.unlock();
    for (auto& k : two.kfs) {
      wr32(out, k->set_pose_calls);
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) wr(out, &k->Tcw.at<float>(r, c), 1);
    }
    for (auto& m : two.mps) {
      wr32(out, m->set_pos_calls);
      wr32(out, m->update_calls);
      for (int r = 0; r < 3; r++) wr(out, &m->pos.at<float>(r), 1);
    }
    long n1 = 0, n2 = 0;
    for (auto& k : two.kfs) n1 += (long)k->erased.size();
    wr32(out, n1);
    for (auto& k : two.kfs)
      for (MapPoint* m : k->erased) {
        wr32(out, (long)k->mnId);
        wr32(out, (long)m->mnId);
      }
    for (auto& m : two.mps) n2 += (long)m->erased.size();
    wr32(out, n2);
    for (auto& m : two.mps)
      for (KeyFrame* k : m->erased) {
        wr32(out, (long)k->mnId);
        wr32(out, (long)m->mnId);
      }
    for (auto& k : two.kfs)
      for (auto& m : two.mps) {
        bool has = false;
        for (MapPoint* q : k->mvpMapPoints) has = has || q == m.get();
        fputc(has ? 1 : 0, out);
      }
    for (auto& m : two.mps)
      for (auto& k : two.kfs) fputc(m->observations.count(k.get()) ? 1 : 0, out);
  }
  fclose(out);
  return 0;
}
