// KeyFrameDatabase_hip.h -- host-side adapter with the public surface of ORB_SLAM2::KeyFrameDatabase on liborbfe.
//
// The reference's class (Source/Libraries/ORB_SLAM2/src/KeyFrameDatabase.cc) keeps an inverted file of KeyFrame pointers on the host
// and walks it per query.  This class keeps the BoW vectors in device memory behind an orbfe_kfdb handle (include/orbfe.h) and asks
// the library for the candidates; it hands back the same KeyFrame pointers in the same order.
//
// The library needs each keyframe's GetBestCovisibilityKeyFrames(10) as a row of ids.  Two modes:
//   polling (default)   before every query the adapter calls GetBestCovisibilityKeyFrames(10) on every keyframe in the database,
//                       compares the row with the one it sent last and uploads the rows that changed.  The host program needs no
//                       change; a query costs one such call per keyframe on the host.
//   notified            the host program calls NotifyConnectionsChanged(pKF) wherever it changes a keyframe's covisibility graph
//                       (KeyFrame::UpdateConnections, UpdateBestCovisibles, EraseConnection, SetBadFlag); only those rows and the
//                       rows of newly added keyframes are read before a query.  A missed notification gives stale neighbours.
// Deviation from the reference: mRelocScore starts at 0 when a keyframe is added (the reference leaves it uninitialised).
//
// A template over the KeyFrame and Frame types so that it compiles (and is unit-tested, tests/cpp_kfdb) without the reference tree.
// A failing library call is logged to stderr, never thrown: without a device both detection functions return an empty vector.
//
// Members used (same names as the reference):
//   KeyFrame: mnId, mBowVec (a map from word id to value), GetBestCovisibilityKeyFrames(int), GetConnectedKeyFrames()
//   Frame:    mBowVec
#pragma once
#include <stdio.h>

#include <algorithm>
#include <array>
#include <set>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../../include/orbfe.h"

namespace ORB_SLAM2 {
namespace orbfe_host {

template <class KeyFrameT, class FrameT>
class KeyFrameDatabase {
 public:
  // n_words = ORBVocabulary::size()
  explicit KeyFrameDatabase(int n_words, int device = -1, bool notified = false) : mbNotified(notified) {
    if (orbfe_kfdb_create(n_words, ORBFE_KFDB_L1_NORM, device, &mpDb) != ORBFE_OK) Log("orbfe_kfdb_create");
  }
  ~KeyFrameDatabase() { orbfe_kfdb_destroy(mpDb); }
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  bool ok() const { return mpDb != nullptr; }

  void add(KeyFrameT* pKF) {
    if (!mpDb) return;
    std::vector<int32_t> ids;
    std::vector<double> vals;
    Unpack(pKF->mBowVec, ids, vals);
    if (orbfe_kfdb_add(mpDb, (int64_t)pKF->mnId, ids.data(), vals.data(), (int)ids.size()) != ORBFE_OK) {
      Log("orbfe_kfdb_add");
      return;
    }
    mKFs[(int64_t)pKF->mnId] = pKF;
    mChanged.insert(pKF);
  }

  void erase(KeyFrameT* pKF) {
    if (!mpDb) return;
    if (orbfe_kfdb_erase(mpDb, (int64_t)pKF->mnId) != ORBFE_OK) Log("orbfe_kfdb_erase");
    mKFs.erase((int64_t)pKF->mnId);
    mChanged.erase(pKF);
  }

  void clear() {
    if (!mpDb) return;
    if (orbfe_kfdb_clear(mpDb) != ORBFE_OK) Log("orbfe_kfdb_clear");
    mKFs.clear();
    mRows.clear();
    mChanged.clear();
  }

  // notified mode: pKF's covisibility graph changed
  void NotifyConnectionsChanged(KeyFrameT* pKF) { mChanged.insert(pKF); }

  std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore) {
    if (!mpDb) return Fail("DetectLoopCandidates: no database (no HIP device)");
    if (!Refresh()) return std::vector<KeyFrameT*>();
    std::vector<int32_t> ids;
    std::vector<double> vals;
    Unpack(pKF->mBowVec, ids, vals);
    std::vector<int64_t> conn;
    for (KeyFrameT* c : pKF->GetConnectedKeyFrames()) conn.push_back((int64_t)c->mnId);
    std::sort(conn.begin(), conn.end());
    conn.erase(std::unique(conn.begin(), conn.end()), conn.end());
    const int32_t q_off[2] = {0, (int32_t)ids.size()}, c_off[2] = {0, (int32_t)conn.size()};
    std::vector<int64_t> cand(std::max<size_t>(mKFs.size(), 1));
    int32_t n = 0;
    if (orbfe_kfdb_detect_loop(mpDb, 1, q_off, ids.data(), vals.data(), &minScore, c_off, conn.data(), (int)cand.size(), cand.data(), &n,
                               nullptr, nullptr, nullptr) != ORBFE_OK)
      return Fail("orbfe_kfdb_detect_loop");
    return Pointers(cand, n);
  }

  std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F) {
    if (!mpDb) return Fail("DetectRelocalizationCandidates: no database (no HIP device)");
    if (!Refresh()) return std::vector<KeyFrameT*>();
    std::vector<int32_t> ids;
    std::vector<double> vals;
    Unpack(F->mBowVec, ids, vals);
    const int32_t q_off[2] = {0, (int32_t)ids.size()};
    std::vector<int64_t> cand(std::max<size_t>(mKFs.size(), 1));
    int32_t n = 0;
    if (orbfe_kfdb_detect_relocalization(mpDb, 1, q_off, ids.data(), vals.data(), (int)cand.size(), cand.data(), &n, nullptr, nullptr,
                                         nullptr) != ORBFE_OK)
      return Fail("orbfe_kfdb_detect_relocalization");
    return Pointers(cand, n);
  }

 private:
  typedef std::array<int64_t, ORBFE_KFDB_NEIGHBOURS> Row;

  template <class BowVectorT>
  static void Unpack(const BowVectorT& v, std::vector<int32_t>& ids, std::vector<double>& vals) {
    ids.reserve(v.size());
    vals.reserve(v.size());
    for (typename BowVectorT::const_iterator it = v.begin(); it != v.end(); ++it) {   // a std::map: ascending word ids
      ids.push_back((int32_t)it->first);
      vals.push_back((double)it->second);
    }
  }

  // uploads the rows that differ from what the library has
  bool Refresh() {
    std::vector<int64_t> kf_ids, rows;
    auto visit = [&](KeyFrameT* pKF) {
      Row row;
      row.fill(-1);
      const std::vector<KeyFrameT*> vpNeighs = pKF->GetBestCovisibilityKeyFrames(ORBFE_KFDB_NEIGHBOURS);
      for (size_t k = 0; k < vpNeighs.size() && k < row.size(); k++) row[k] = (int64_t)vpNeighs[k]->mnId;
      const auto it = mRows.find((int64_t)pKF->mnId);
      if (it != mRows.end() && it->second == row) return;
      mRows[(int64_t)pKF->mnId] = row;
      kf_ids.push_back((int64_t)pKF->mnId);
      rows.insert(rows.end(), row.begin(), row.end());
    };
    if (mbNotified) {
      for (KeyFrameT* pKF : mChanged)
        if (mKFs.count((int64_t)pKF->mnId)) visit(pKF);
    } else {
      for (const auto& kv : mKFs) visit(kv.second);
    }
    mChanged.clear();
    if (kf_ids.empty()) return true;
    if (orbfe_kfdb_set_covisibles(mpDb, (int)kf_ids.size(), kf_ids.data(), rows.data()) != ORBFE_OK) {
      Log("orbfe_kfdb_set_covisibles");
      return false;
    }
    return true;
  }

  std::vector<KeyFrameT*> Pointers(const std::vector<int64_t>& cand, int n) const {
    std::vector<KeyFrameT*> out;
    out.reserve((size_t)std::max(n, 0));
    for (int k = 0; k < n && k < (int)cand.size(); k++) {
      const auto it = mKFs.find(cand[k]);
      if (it != mKFs.end()) out.push_back(it->second);
    }
    return out;
  }

  static void Log(const char* what) { fprintf(stderr, "orbfe_host::KeyFrameDatabase: %s failed: %s\n", what, orbfe_last_error()); }
  static std::vector<KeyFrameT*> Fail(const char* what) {
    Log(what);
    return std::vector<KeyFrameT*>();
  }

  orbfe_kfdb* mpDb = nullptr;
  bool mbNotified;
  std::unordered_map<int64_t, KeyFrameT*> mKFs;   // the live entries
  std::unordered_map<int64_t, Row> mRows;         // the rows the library has
  std::unordered_set<KeyFrameT*> mChanged;
};

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
