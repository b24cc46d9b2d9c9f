// Tracking_hip.h -- host-side adapter of Tracking::UpdateLocalMap: the bodies of Tracking::UpdateLocalKeyFrames and
// Tracking::UpdateLocalPoints (Source/Libraries/ORB_SLAM2/src/Tracking.cc:1115-1214, :1090-1113) in ONE marshal, the vote
// (orbfe_covis_count) and ONE call of orbfe_local_map (include/orbfe.h), which also returns what the first half of
// Tracking::SearchLocalPoints (:1036-1049, :1057-1060) decides: each local point's skip.
//
// UpdateLocalMap marshals the frame's points with their observations, the keyframes those name and, of each of them,
// GetBestCovisibilityKeyFrames(10), GetChilds() and GetParent() -- rows sorted by pointer, so that a row's index IS its position in the
// reference's std::map<KeyFrame*, ...> and std::set<KeyFrame*>, as Covisibility_hip.h does -- and the slot vectors of all those rows.
// Afterwards it writes what the reference writes: bad points leave the frame (:1127-1129), the two vectors are filled in the
// reference's order, mnTrackReferenceForFrame is set on the listed keyframes and points, pRefKF is the keyframe that shares most
// points (left alone when every voted keyframe is bad, :1211).  With the caller stay mCurrentFrame.mpReferenceKF = pRefKF and
// mpMap->SetReferenceMapPoints.
//
// vpAlsoSeen: the points whose mnLastFrameSeen is the frame's id although the frame does not hold them any more -- the outliers
// TrackWithMotionModel / TrackReferenceKeyFrame discarded (:711, :825).  pvSkip (optional): one byte per local point, 1 when
// SearchLocalPoints passes it over (`mnLastFrameSeen == mCurrentFrame.mnId`); with it the caller fills orbfe_map_point.skip without
// touching mnLastFrameSeen.  IncreaseVisible() on the frame's own points (:1044) stays with the caller.
//
// Returns 1; 0 for the reference's early return (nothing voted: bad points have left the frame, the vectors and pRefKF are as they
// were); -1 with a line on stderr when a call failed or the frame was refused or needs more room than one call has
// (ORBFE_COV_MAX_CONN voted keyframes), and then every object is as it was.  A template over the KeyFrame type so that it compiles
// (and is unit-tested, tests/cpp_localmap) without the reference tree.
//
// Members used (same names as the reference):
//   KeyFrame: GetMapPointMatches(), isBad(), GetBestCovisibilityKeyFrames(), GetChilds(), GetParent(), mnTrackReferenceForFrame
//   MapPoint: isBad(), GetObservations(), mnTrackReferenceForFrame
//   Frame:    N, mvpMapPoints, mnId
#pragma once
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <type_traits>
#include <vector>

#include "../../../include/orbfe.h"

namespace ORB_SLAM2 {
namespace orbfe_host {

template <class KeyFrameT>
struct LocalMap {
  typedef typename std::remove_pointer<typename decltype(std::declval<KeyFrameT>().GetMapPointMatches())::value_type>::type MapPointT;
  typedef decltype(std::declval<MapPointT>().GetObservations()) ObservationsT;

  struct Neighbours {
    std::vector<KeyFrameT*> best;
    std::set<KeyFrameT*> children;
    KeyFrameT* parent;
  };

  template <class FrameT>
  static int UpdateLocalMap(FrameT& F, std::vector<KeyFrameT*>& vpLocalKeyFrames, std::vector<MapPointT*>& vpLocalMapPoints, KeyFrameT*& pRefKF,
                            const std::vector<MapPointT*>& vpAlsoSeen, std::vector<uint8_t>* pvSkip) {
    // the points: index by first sight; only the frame's own carry their observations
    std::map<MapPointT*, int32_t> point_of;
    std::vector<MapPointT*> point;
    std::vector<uint8_t> point_bad;
    auto index_of = [&](MapPointT* pMP) {
      typename std::map<MapPointT*, int32_t>::iterator it = point_of.find(pMP);
      if (it != point_of.end()) return it->second;
      point_of[pMP] = (int32_t)point.size();
      point.push_back(pMP);
      point_bad.push_back(pMP->isBad() ? 1 : 0);
      return (int32_t)point.size() - 1;
    };
    std::vector<int32_t> frame_slots;
    for (int i = 0; i < F.N; i++) frame_slots.push_back(F.mvpMapPoints[i] ? index_of(F.mvpMapPoints[i]) : -1);
    const size_t n_frame_points = point.size();
    std::vector<ObservationsT> observations(n_frame_points);
    std::map<KeyFrameT*, int32_t> row_of;   // iterates in pointer order: row == kf_order
    for (size_t p = 0; p < n_frame_points; p++) {
      if (!point_bad[p]) observations[p] = point[p]->GetObservations();
      for (typename ObservationsT::const_iterator mit = observations[p].begin(); mit != observations[p].end(); ++mit) row_of[mit->first] = 0;
    }
    // the graph around the keyframes that can be voted
    std::map<KeyFrameT*, Neighbours> around;
    std::vector<KeyFrameT*> voters;
    for (typename std::map<KeyFrameT*, int32_t>::iterator it = row_of.begin(); it != row_of.end(); ++it) voters.push_back(it->first);
    for (KeyFrameT* pKF : voters) {
      if (pKF->isBad()) continue;   // never listed, so never expanded
      Neighbours& G = around[pKF];
      G.best = pKF->GetBestCovisibilityKeyFrames(ORBFE_LM_BEST);
      G.children = pKF->GetChilds();
      G.parent = pKF->GetParent();
      for (KeyFrameT* b : G.best) row_of[b] = 0;
      for (KeyFrameT* c : G.children) row_of[c] = 0;
      if (G.parent) row_of[G.parent] = 0;
    }
    std::vector<KeyFrameT*> kf;
    for (typename std::map<KeyFrameT*, int32_t>::iterator it = row_of.begin(); it != row_of.end(); ++it) {
      it->second = (int32_t)kf.size();
      kf.push_back(it->first);
    }
    const size_t n_kf = kf.size();
    std::vector<orbfe_lm_graph> graph(n_kf);
    std::vector<int32_t> children, order(n_kf);
    std::vector<uint8_t> kf_bad(n_kf);
    std::vector<std::vector<int32_t> > kf_slots(n_kf);
    std::vector<orbfe_cov_keyframe> table(n_kf);
    for (size_t r = 0; r < n_kf; r++) {
      order[r] = (int32_t)r;
      kf_bad[r] = kf[r]->isBad() ? 1 : 0;
      orbfe_lm_graph& G = graph[r];
      memset(&G, 0, sizeof(G));
      G.parent = -1;
      G.child_offset = (int32_t)children.size();
      typename std::map<KeyFrameT*, Neighbours>::iterator it = around.find(kf[r]);
      if (it != around.end()) {
        G.parent = it->second.parent ? row_of[it->second.parent] : -1;
        for (KeyFrameT* c : it->second.children) children.push_back(row_of[c]);   // set order is pointer order is row order
        G.n_children = (int32_t)children.size() - G.child_offset;
        for (KeyFrameT* b : it->second.best) G.best[G.n_best++] = row_of[b];
      }
      for (MapPointT* pMP : kf[r]->GetMapPointMatches()) kf_slots[r].push_back(pMP ? index_of(pMP) : -1);
      memset(&table[r], 0, sizeof(table[r]));
      table[r].n_keys = (int32_t)kf_slots[r].size();
      table[r].slots = (uint64_t)(uintptr_t)kf_slots[r].data();
    }
    std::vector<int32_t> seen;
    for (MapPointT* pMP : vpAlsoSeen)
      if (pMP) seen.push_back(index_of(pMP));
    const size_t n_points = point.size();
    std::vector<orbfe_mp_obs> obs;
    std::vector<orbfe_mp_point> lists(n_points);
    for (size_t p = 0; p < n_points; p++) {
      memset(&lists[p], 0, sizeof(lists[p]));
      lists[p].obs_offset = (int32_t)obs.size();
      if (p >= n_frame_points) continue;
      for (typename ObservationsT::const_iterator mit = observations[p].begin(); mit != observations[p].end(); ++mit) {
        orbfe_mp_obs o;
        o.kf = row_of[mit->first];
        o.idx = (int32_t)mit->second;
        obs.push_back(o);
      }
      lists[p].n_obs = (int32_t)obs.size() - lists[p].obs_offset;
    }

    orbfe_cov_subject S;
    S.slot_offset = 0; S.n_slots = (int32_t)frame_slots.size(); S.self = -1; S.mode = ORBFE_COV_VOTES;
    const int conn_cap = (int)std::max<size_t>(1, std::min<size_t>(n_kf, ORBFE_COV_MAX_CONN));
    orbfe_cov_header vote;
    std::vector<orbfe_cov_entry> entries((size_t)conn_cap);
    int rc = orbfe_covis_count(obs.data(), (int)obs.size(), lists.data(), point_bad.data(), (int)n_points, order.data(), kf_bad.data(), (int)n_kf,
                               frame_slots.data(), (int)frame_slots.size(), &S, 1, conn_cap, &vote, entries.data());
    if (rc != ORBFE_OK) {
      fprintf(stderr, "orbfe_host::UpdateLocalMap: orbfe_covis_count failed: %s (code %d)\n", orbfe_last_error(), rc);
      return -1;
    }
    const int kf_cap = (int)std::max<size_t>(1, std::min<size_t>(n_kf, ORBFE_LM_MAX_KF_CAP)), p_cap = (int)std::max<size_t>(1, n_points);
    orbfe_lm_frame frame;
    frame.seen_offset = 0; frame.n_seen = (int32_t)seen.size();
    orbfe_lm_header H;
    std::vector<int32_t> local_kf((size_t)kf_cap), local_points((size_t)p_cap);
    std::vector<orbfe_map_point> records(pvSkip ? n_points : 0), map_points(pvSkip ? (size_t)p_cap : 0);   // only `skip` is wanted of them
    if (pvSkip && n_points) memset(records.data(), 0, n_points * sizeof(orbfe_map_point));
    int32_t n_out = 0;
    rc = orbfe_local_map(&vote, entries.data(), conn_cap, graph.data(), children.data(), (int)children.size(), table.data(), kf_bad.data(),
                         (int)n_kf, point_bad.data(), (int)n_points, frame_slots.data(), (int)frame_slots.size(), &S, &frame, seen.data(),
                         (int)seen.size(), pvSkip && n_points ? records.data() : NULL, 1, kf_cap, p_cap, &H, local_kf.data(), local_points.data(),
                         &n_out, pvSkip && n_points ? map_points.data() : NULL);
    if (rc != ORBFE_OK) {
      fprintf(stderr, "orbfe_host::UpdateLocalMap: orbfe_local_map failed: %s (code %d)\n", orbfe_last_error(), rc);
      return -1;
    }
    if (H.status != ORBFE_LM_OK && H.status != ORBFE_LM_EMPTY) {
      fprintf(stderr, "orbfe_host::UpdateLocalMap: the frame was %s\n",
              vote.status == ORBFE_COV_OVERFLOW ? "voted into more keyframes than one call orders" : "refused");
      return -1;
    }
    for (int i = 0; i < F.N; i++)   // only once the calls have succeeded, so that a failure leaves the frame as it was
      if (frame_slots[i] >= 0 && point_bad[frame_slots[i]]) F.mvpMapPoints[i] = static_cast<MapPointT*>(NULL);   // :1127-1129
    if (H.status == ORBFE_LM_EMPTY) return 0;   // :1133-1134
    vpLocalKeyFrames.clear();
    vpLocalKeyFrames.reserve(3 * (size_t)vote.n_counted);
    for (int j = 0; j < H.n_local_kf; j++) {
      vpLocalKeyFrames.push_back(kf[local_kf[j]]);
      kf[local_kf[j]]->mnTrackReferenceForFrame = F.mnId;
    }
    if (H.ref_kf >= 0) pRefKF = kf[H.ref_kf];   // :1211
    vpLocalMapPoints.clear();
    if (pvSkip) pvSkip->clear();
    for (int e = 0; e < H.n_local_points; e++) {
      vpLocalMapPoints.push_back(point[local_points[e]]);
      point[local_points[e]]->mnTrackReferenceForFrame = F.mnId;
      if (pvSkip) pvSkip->push_back(map_points[e].skip ? 1 : 0);
    }
    return 1;
  }
};

template <class KeyFrameT, class FrameT, class MapPointT>
int UpdateLocalMap(FrameT& F, std::vector<KeyFrameT*>& vpLocalKeyFrames, std::vector<MapPointT*>& vpLocalMapPoints, KeyFrameT*& pRefKF,
                   const std::vector<MapPointT*>& vpAlsoSeen, std::vector<uint8_t>* pvSkip = NULL) {
  return LocalMap<KeyFrameT>::UpdateLocalMap(F, vpLocalKeyFrames, vpLocalMapPoints, pRefKF, vpAlsoSeen, pvSkip);
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
