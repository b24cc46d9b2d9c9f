// test_kfdb_dropin.cpp -- runs a scripted sequence of add, erase, graph changes and both kinds of query through
// orbfe_host::KeyFrameDatabase on the mock KeyFrame / Frame and writes every query's candidate ids, for tests/test_kfdb_dropin_cpp.py.
//   script (little endian): int32 n_words, notified, n_ops; per op an int32 code and
//     0 make   int64 id, int32 n, int32 ids[n], double vals[n]      a KeyFrame object that is in no database yet
//     1 add    int64 id            2 erase  int64 id            3 clear
//     4 graph  int64 id, int64 neigh[10] (-1 pads), int32 n_conn, int64 conn[n_conn]   (+ NotifyConnectionsChanged in notified mode)
//     5 reloc  int32 n, int32 ids[n], double vals[n]
//     6 loop   int64 id, float min_score
//   output: per query int32 n, int64 ids[n].  Exit code 3 when the database could not be created (no device): every query still
//   ran and returned nothing.
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <memory>
#include <vector>

#include "mock/KeyFrame.h"
#include "../../refactored_orb_slam2_amd/csrc/host/KeyFrameDatabase_hip.h"

using ORB_SLAM2::Frame;
using ORB_SLAM2::KeyFrame;

template <class T>
static bool rd(FILE* f, T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

static bool read_vector(FILE* f, DBoW2::BowVector& v) {
  int32_t n;
  if (!rd(f, &n) || n < 0) return false;
  std::vector<int32_t> ids((size_t)n);
  std::vector<double> vals((size_t)n);
  if (n && (!rd(f, ids.data(), (size_t)n) || !rd(f, vals.data(), (size_t)n))) return false;
  for (int i = 0; i < n; i++) v[(DBoW2::WordId)ids[i]] = vals[i];
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t n_words, notified, n_ops;
  if (!rd(in, &n_words) || !rd(in, &notified) || !rd(in, &n_ops)) return 2;
  ORB_SLAM2::orbfe_host::KeyFrameDatabase<KeyFrame, Frame> db(n_words, -1, notified != 0);
  std::map<int64_t, std::unique_ptr<KeyFrame>> kfs;
  auto kf = [&](int64_t id) {
    std::unique_ptr<KeyFrame>& p = kfs[id];
    if (!p) {
      p.reset(new KeyFrame);
      p->mnId = (long unsigned int)id;
    }
    return p.get();
  };
  auto emit = [&](const std::vector<KeyFrame*>& v) {
    const int32_t n = (int32_t)v.size();
    fwrite(&n, 4, 1, out);
    for (KeyFrame* p : v) {
      const int64_t id = (int64_t)p->mnId;
      fwrite(&id, 8, 1, out);
    }
  };
  for (int op = 0; op < n_ops; op++) {
    int32_t code;
    int64_t id = 0;
    if (!rd(in, &code)) return 2;
    if (code == 0) {
      if (!rd(in, &id)) return 2;
      KeyFrame* p = kf(id);
      p->mBowVec.clear();
      if (!read_vector(in, p->mBowVec)) return 2;
    } else if (code == 1 || code == 2) {
      if (!rd(in, &id)) return 2;
      if (code == 1) db.add(kf(id)); else db.erase(kf(id));
    } else if (code == 3) {
      db.clear();
    } else if (code == 4) {
      int64_t neigh[10];
      int32_t n_conn;
      if (!rd(in, &id) || !rd(in, neigh, 10) || !rd(in, &n_conn) || n_conn < 0) return 2;
      std::vector<int64_t> conn((size_t)n_conn);
      if (n_conn && !rd(in, conn.data(), (size_t)n_conn)) return 2;
      KeyFrame* p = kf(id);
      p->mvpOrderedConnectedKeyFrames.clear();
      for (int k = 0; k < 10 && neigh[k] >= 0; k++) p->mvpOrderedConnectedKeyFrames.push_back(kf(neigh[k]));
      p->mspConnected.clear();
      for (int64_t c : conn) p->mspConnected.insert(kf(c));
      if (notified) db.NotifyConnectionsChanged(p);
    } else if (code == 5) {
      Frame F;
      if (!read_vector(in, F.mBowVec)) return 2;
      emit(db.DetectRelocalizationCandidates(&F));
    } else if (code == 6) {
      float min_score;
      if (!rd(in, &id) || !rd(in, &min_score)) return 2;
      emit(db.DetectLoopCandidates(kf(id), min_score));
    } else {
      return 2;
    }
  }
  fclose(out);
  fclose(in);
  return db.ok() ? 0 : 3;
}
