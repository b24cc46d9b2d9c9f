// Covisibility_hip.h -- host-side adapter of the covisibility graph: KeyFrame::UpdateConnections for a vector of keyframes, the vote
// of Tracking::UpdateLocalKeyFrames for a frame, and LocalMapping::KeyFrameCulling, each in ONE call of liborbfe (include/orbfe.h:
// orbfe_covis_count, orbfe_covis_cull_keyframes).
//
// The reference walks a std::map per map point in all three (Source/Libraries/ORB_SLAM2/src/KeyFrame.cc:268-354, Tracking.cc:1115-1159,
// LocalMapping.cc:595-655).  The functions here marshal the map once -- the points of the subjects' mvpMapPoints, their observations
// in map order, and the keyframes those name, as rows sorted by pointer so that a row's index IS its position in the reference's
// std::map<KeyFrame*, ...> --, ask the library, and replay on the objects, in the reference's order, what the library leaves to the
// caller: AddConnection on the other keyframes, the weights map and the ordered vectors, the first-connection parent;
// mnTrackReferenceForFrame and the bad points cleared out of the frame; SetBadFlag on the redundant keyframes.
//
// Templates over the KeyFrame type (the MapPoint type is the element of its mvpMapPoints) so that they compile (and are unit-tested,
// tests/cpp_covis) without the reference tree.  A failing library call is logged to stderr, never thrown, and leaves every object as it
// was, with one exception: a keyframe or frame with more than ORBFE_COV_MAX_CONN (2 048) counted keyframes cannot be ordered by one
// call (status OVERFLOW); UpdateConnectionsBatch logs it and leaves THAT keyframe's connections as they were (the others of the vector
// are updated), VoteLocalKeyFrames returns -1.  The reference has no such bound; a host whose graph can grow that dense keeps the
// reference's loop for those keyframes.  What is read goes through the reference's own locking accessors; mbNotErase is read, and the connection members are written,
// under mMutexConnections, as the reference does.  Those members are protected in the reference: declare
//     template <class T> friend struct orbfe_host::Covisibility;
// in class KeyFrame.
//
// Members used (same names as the reference):
//   KeyFrame: mnId, GetMapPointMatches(), isBad(), AddConnection(), AddChild(), GetVectorCovisibleKeyFrames(), SetBadFlag(), mvKeysUn,
//             mvuRight, mvDepth, mThDepth, mbNotErase, mMutexConnections, mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames,
//             mvOrderedWeights, mbFirstConnection, mpParent, mnTrackReferenceForFrame
//   MapPoint: isBad(), GetObservations(), Observations()
//   Frame:    N, mvpMapPoints, mnId
#pragma once
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../../include/orbfe.h"

namespace ORB_SLAM2 {
namespace orbfe_host {

template <class KeyFrameT>
struct Covisibility {
  typedef typename std::remove_pointer<typename decltype(std::declval<KeyFrameT>().GetMapPointMatches())::value_type>::type MapPointT;
  typedef decltype(std::declval<MapPointT>().GetObservations()) ObservationsT;

  // the map as the library takes it
  struct Tables {
    std::map<MapPointT*, int32_t> point_of;
    std::vector<ObservationsT> observations;   // per point; empty for a bad one
    std::vector<uint8_t> point_bad;
    std::vector<int32_t> weighted;
    std::map<KeyFrameT*, int32_t> row_of;      // iterates in pointer order: row == kf_order
    std::vector<KeyFrameT*> kf;
    std::vector<orbfe_mp_obs> obs;
    std::vector<orbfe_mp_point> points;

    // the slots of one mvpMapPoints vector; every point seen for the first time is read under its own locks
    void Slots(const std::vector<MapPointT*>& vpMP, std::vector<int32_t>& slots) {
      for (MapPointT* pMP : vpMP) {
        if (!pMP) { slots.push_back(-1); continue; }
        typename std::map<MapPointT*, int32_t>::iterator it = point_of.find(pMP);
        if (it == point_of.end()) {
          it = point_of.insert(std::make_pair(pMP, (int32_t)observations.size())).first;
          const bool bad = pMP->isBad();
          point_bad.push_back(bad ? 1 : 0);
          observations.push_back(bad ? ObservationsT() : pMP->GetObservations());
          weighted.push_back(bad ? 0 : pMP->Observations());
          for (typename ObservationsT::const_iterator mit = observations.back().begin(); mit != observations.back().end(); ++mit)
            row_of[mit->first] = 0;
        }
        slots.push_back(it->second);
      }
    }
    // after the last Slots(): rows in pointer order, the observation array in map order
    void Finish() {
      int32_t r = 0;
      for (typename std::map<KeyFrameT*, int32_t>::iterator it = row_of.begin(); it != row_of.end(); ++it, ++r) {
        it->second = r;
        kf.push_back(it->first);
      }
      for (const ObservationsT& O : observations) {
        orbfe_mp_point Q;
        memset(&Q, 0, sizeof(Q));
        Q.obs_offset = (int32_t)obs.size();
        Q.n_obs = (int32_t)O.size();
        for (typename ObservationsT::const_iterator mit = O.begin(); mit != O.end(); ++mit) {
          orbfe_mp_obs o;
          o.kf = row_of[mit->first];
          o.idx = (int32_t)mit->second;
          obs.push_back(o);
        }
        points.push_back(Q);
      }
    }
  };

  static bool Count(Tables& T, const std::vector<int32_t>& slots, const std::vector<orbfe_cov_subject>& subjects, int conn_cap,
                    std::vector<orbfe_cov_header>& headers, std::vector<orbfe_cov_entry>& entries, const char* who) {
    std::vector<int32_t> order(T.kf.size());
    std::vector<uint8_t> kf_bad(T.kf.size());
    for (size_t r = 0; r < T.kf.size(); r++) {
      order[r] = (int32_t)r;
      kf_bad[r] = T.kf[r]->isBad() ? 1 : 0;
    }
    headers.resize(subjects.size());
    entries.resize(subjects.size() * (size_t)conn_cap);
    const int rc = orbfe_covis_count(T.obs.data(), (int)T.obs.size(), T.points.data(), T.point_bad.data(), (int)T.points.size(), order.data(),
                                     kf_bad.data(), (int)T.kf.size(), slots.data(), (int)slots.size(), subjects.data(), (int)subjects.size(),
                                     conn_cap, headers.data(), entries.data());
    if (rc != ORBFE_OK) fprintf(stderr, "orbfe_host::%s: orbfe_covis_count failed: %s (code %d)\n", who, orbfe_last_error(), rc);
    return rc == ORBFE_OK;
  }
  static int ConnCap(const Tables& T) {
    return (int)std::max<size_t>(1, std::min<size_t>(T.kf.size(), ORBFE_COV_MAX_CONN));
  }

  // pKF->UpdateConnections() for every keyframe of the vector, in its order.  Returns the number updated, -1 when the call failed.
  static int UpdateConnectionsBatch(const std::vector<KeyFrameT*>& vpKFs) {
    Tables T;
    std::vector<int32_t> slots;
    std::vector<orbfe_cov_subject> subjects;
    std::vector<KeyFrameT*> taken;
    for (KeyFrameT* pKF : vpKFs) {
      if (!pKF) continue;
      orbfe_cov_subject S;
      S.slot_offset = (int32_t)slots.size();
      T.Slots(pKF->GetMapPointMatches(), slots);
      S.n_slots = (int32_t)slots.size() - S.slot_offset;
      S.self = 0;
      S.mode = ORBFE_COV_CONNECTIONS;
      T.row_of[pKF] = 0;
      subjects.push_back(S);
      taken.push_back(pKF);
    }
    if (taken.empty()) return 0;
    T.Finish();
    for (size_t s = 0; s < taken.size(); s++) subjects[s].self = T.row_of[taken[s]];
    const int cap = ConnCap(T);
    std::vector<orbfe_cov_header> headers;
    std::vector<orbfe_cov_entry> entries;
    if (!Count(T, slots, subjects, cap, headers, entries, "UpdateConnectionsBatch")) return -1;
    int n = 0;
    for (size_t s = 0; s < taken.size(); s++) {
      const orbfe_cov_header& H = headers[s];
      const orbfe_cov_entry* E = entries.data() + s * (size_t)cap;
      KeyFrameT* pKF = taken[s];
      if (H.status == ORBFE_COV_EMPTY) continue;   // :302-303
      if (H.status != ORBFE_COV_OK) {
        fprintf(stderr, "orbfe_host::UpdateConnectionsBatch: a keyframe was %s; it is left alone\n",
                H.status == ORBFE_COV_OVERFLOW ? "connected to more keyframes than one call orders" : "refused");
        continue;
      }
      // :314-330: the other keyframes hear of it in map order, which is row order
      std::vector<orbfe_cov_entry> told(E, E + H.n_ordered);
      if (H.single) { told.resize(1); told[0].kf = H.kf_max; told[0].weight = H.w_max; }
      std::vector<orbfe_cov_entry> in_map_order(told);
      std::sort(in_map_order.begin(), in_map_order.end(), [](const orbfe_cov_entry& a, const orbfe_cov_entry& b) { return a.kf < b.kf; });
      for (const orbfe_cov_entry& e : in_map_order) T.kf[e.kf]->AddConnection(pKF, e.weight);
      std::map<KeyFrameT*, int> KFcounter;
      for (int e = 0; e < H.n_written; e++) KFcounter[T.kf[E[e].kf]] = E[e].weight;
      std::unique_lock<std::mutex> lockCon(pKF->mMutexConnections);
      pKF->mConnectedKeyFrameWeights = KFcounter;
      pKF->mvpOrderedConnectedKeyFrames.clear();
      pKF->mvOrderedWeights.clear();
      for (const orbfe_cov_entry& e : told) {
        pKF->mvpOrderedConnectedKeyFrames.push_back(T.kf[e.kf]);
        pKF->mvOrderedWeights.push_back(e.weight);
      }
      if (pKF->mbFirstConnection && pKF->mnId != 0) {
        pKF->mpParent = pKF->mvpOrderedConnectedKeyFrames.front();
        pKF->mpParent->AddChild(pKF);
        pKF->mbFirstConnection = false;
      }
      n++;
    }
    return n;
  }

  // The vote of Tracking::UpdateLocalKeyFrames (:1117-1159): bad points leave the frame, vpLocalKeyFrames is cleared and filled as
  // the vote fills mvpLocalKeyFrames, pKFmax is the keyframe that shares most points (NULL: every voted keyframe is bad).  Returns 1;
  // 0 for the early return (nothing voted: vpLocalKeyFrames is not touched); -1 when the call failed.  The expansion by neighbours,
  // children and parents (:1161-1220) stays with the caller.
  template <class FrameT>
  static int VoteLocalKeyFrames(FrameT& F, std::vector<KeyFrameT*>& vpLocalKeyFrames, KeyFrameT*& pKFmax) {
    Tables T;
    std::vector<int32_t> slots;
    std::vector<MapPointT*> vpMP(F.mvpMapPoints.begin(), F.mvpMapPoints.begin() + F.N);
    T.Slots(vpMP, slots);
    T.Finish();
    orbfe_cov_subject S;
    S.slot_offset = 0; S.n_slots = (int32_t)slots.size(); S.self = -1; S.mode = ORBFE_COV_VOTES;
    std::vector<orbfe_cov_subject> subjects(1, S);
    const int cap = ConnCap(T);
    std::vector<orbfe_cov_header> headers;
    std::vector<orbfe_cov_entry> entries;
    if (!Count(T, slots, subjects, cap, headers, entries, "VoteLocalKeyFrames")) return -1;
    const orbfe_cov_header& H = headers[0];
    for (int i = 0; i < F.N; i++)   // only once the call has succeeded, so that a failure leaves the frame as it was
      if (slots[i] >= 0 && T.point_bad[slots[i]]) F.mvpMapPoints[i] = static_cast<MapPointT*>(NULL);   // :1127-1129
    if (H.status == ORBFE_COV_EMPTY) return 0;   // :1133-1134
    if (H.status != ORBFE_COV_OK) {
      fprintf(stderr, "orbfe_host::VoteLocalKeyFrames: the frame was %s\n", H.status == ORBFE_COV_OVERFLOW ? "voted into more keyframes than one call orders" : "refused");
      return -1;
    }
    vpLocalKeyFrames.clear();
    vpLocalKeyFrames.reserve(3 * (size_t)H.n_counted);
    for (int e = 0; e < H.n_written; e++) {
      KeyFrameT* pKF = T.kf[entries[e].kf];
      vpLocalKeyFrames.push_back(pKF);
      pKF->mnTrackReferenceForFrame = F.mnId;
    }
    pKFmax = H.kf_max >= 0 ? T.kf[H.kf_max] : static_cast<KeyFrameT*>(NULL);
    return 1;
  }

  // LocalMapping::KeyFrameCulling for pCurrentKF: one call decides every local keyframe with the carry-over of the earlier culls, then
  // SetBadFlag() runs on the redundant ones in order.  Returns the number of keyframes SetBadFlag() was called on, -1 when the call failed.
  static int KeyFrameCulling(KeyFrameT* pCurrentKF, bool bMonocular) {
    const std::vector<KeyFrameT*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
    if (vpLocalKeyFrames.empty()) return 0;
    Tables T;
    std::vector<std::vector<int32_t> > slots(vpLocalKeyFrames.size());
    for (size_t j = 0; j < vpLocalKeyFrames.size(); j++) {
      T.Slots(vpLocalKeyFrames[j]->GetMapPointMatches(), slots[j]);
      T.row_of[vpLocalKeyFrames[j]] = 0;
    }
    T.Finish();
    std::vector<orbfe_cov_keyframe> table(T.kf.size());
    for (size_t r = 0; r < T.kf.size(); r++) {
      KeyFrameT* pKF = T.kf[r];
      orbfe_cov_keyframe& K = table[r];
      memset(&K, 0, sizeof(K));
      K.n_keys = (int32_t)pKF->mvKeysUn.size();
      K.keys_un = (uint64_t)(uintptr_t)pKF->mvKeysUn.data();
      K.u_right = pKF->mvuRight.size() == pKF->mvKeysUn.size() ? (uint64_t)(uintptr_t)pKF->mvuRight.data() : 0;
      K.depth = pKF->mvDepth.size() == pKF->mvKeysUn.size() ? (uint64_t)(uintptr_t)pKF->mvDepth.data() : 0;
      K.th_depth = pKF->mThDepth;
      std::unique_lock<std::mutex> lock(pKF->mMutexConnections);
      K.flags = (pKF->mnId == 0 ? ORBFE_COV_IS_ID0 : 0) | (pKF->mbNotErase ? ORBFE_COV_NOT_ERASE : 0);
    }
    std::vector<int32_t> local(vpLocalKeyFrames.size());
    for (size_t j = 0; j < vpLocalKeyFrames.size(); j++) {
      local[j] = T.row_of[vpLocalKeyFrames[j]];
      slots[j].resize(vpLocalKeyFrames[j]->mvKeysUn.size(), -1);
      table[local[j]].slots = (uint64_t)(uintptr_t)slots[j].data();
    }
    orbfe_cov_problem P;
    P.local_offset = 0; P.n_local = (int32_t)local.size(); P.monocular = bMonocular ? 1 : 0; P.reserved = 0;
    std::vector<orbfe_cov_verdict> verdicts(local.size());
    const int rc = orbfe_covis_cull_keyframes(T.obs.data(), (int)T.obs.size(), T.points.data(), T.point_bad.data(), T.weighted.data(),
                                              (int)T.points.size(), table.data(), (int)table.size(), local.data(), (int)local.size(), &P, 1,
                                              verdicts.data());
    if (rc != ORBFE_OK) {
      fprintf(stderr, "orbfe_host::KeyFrameCulling: orbfe_covis_cull_keyframes failed: %s (code %d)\n", orbfe_last_error(), rc);
      return -1;
    }
    int n = 0;
    for (size_t j = 0; j < local.size(); j++) {
      if (verdicts[j].verdict == ORBFE_COV_ROW_REFUSED)
        fprintf(stderr, "orbfe_host::KeyFrameCulling: a local keyframe was refused; it is left alone\n");
      if (verdicts[j].verdict != ORBFE_COV_CULLED && verdicts[j].verdict != ORBFE_COV_MARKED) continue;
      vpLocalKeyFrames[j]->SetBadFlag();   // :652-653
      n++;
    }
    return n;
  }
};

template <class KeyFrameT>
int UpdateConnectionsBatch(const std::vector<KeyFrameT*>& vpKFs) { return Covisibility<KeyFrameT>::UpdateConnectionsBatch(vpKFs); }
template <class KeyFrameT, class FrameT>
int VoteLocalKeyFrames(FrameT& F, std::vector<KeyFrameT*>& vpLocalKeyFrames, KeyFrameT*& pKFmax) {
  return Covisibility<KeyFrameT>::VoteLocalKeyFrames(F, vpLocalKeyFrames, pKFmax);
}
template <class KeyFrameT>
int KeyFrameCulling(KeyFrameT* pCurrentKF, bool bMonocular) { return Covisibility<KeyFrameT>::KeyFrameCulling(pCurrentKF, bMonocular); }

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
