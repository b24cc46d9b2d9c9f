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
//
// The keyframe decision and the close stereo points (Tracking.cc:851-877, :880-962, :973-1024, :732-777, :455-479): NeedNewKeyFrame,
// CreateNewKeyFramePoints, UpdateLastFramePoints and StereoInitializationPoints marshal ONE frame, make ONE call of
// orbfe_keyframe_insertion and then do on the real objects what the reference does, in its order.  What Tracking holds beside the
// frame comes in a KeyFrameState.
//   NeedNewKeyFrame          the count of :854-866 (into *pnMatchesInliers; IncreaseFound and the stereo sensor's clearing of outlier
//                            slots, :857 and :863-864, stay with the caller and come first), the verdict of :870-877 (into *pbTrackOK)
//                            and the return value of :880-961; mpLocalMapper->InterruptBA() is called where :951 is reached
//   CreateNewKeyFramePoints  :973-1024 for the keyframe pKF made from the frame (nothing for a monocular sensor, :973): per created entry, in creation order, the slot of a
//                            temporal point is cleared, then new MapPoint(x3D, pKF, pMap), AddObservation, pKF->AddMapPoint,
//                            ComputeDistinctiveDescriptors, UpdateNormalAndDepth, pMap->AddMapPoint, the slot.  SetNotStop, new KeyFrame,
//                            InsertKeyFrame and the ids stay with the caller
//   UpdateLastFramePoints    :732-777 (the caller tests :728-730): new MapPoint(x3D, pMap, &LastFrame, i), the slot,
//                            mlpTemporalPoints.push_back
//   StereoInitializationPoints  :466-479 for pKFini (the caller tests N > 500 or lets the call do it: nothing is created otherwise)
// x3D is the frame's own UnprojectStereo(i), as in the reference; the library decides which i, in which order.  Each returns the
// number of points created (NeedNewKeyFrame: 1 or 0), or -1 with a line on stderr when the call failed or the frame was refused,
// and then every object is as it was.
// Members used beside the above:
//   Frame:        mvDepth, mvbOutlier, mvKeysUn, mDescriptors.ptr(0), mvScaleFactors, GetRotationInverse() / GetCameraCenter() (at<float>),
//                 cx, cy, invfx, invfy, UnprojectStereo(i)
//   KeyFrame:     AddMapPoint(pMP, i)
//   MapPoint:     Observations(), the two constructors, AddObservation(pKF, i), ComputeDistinctiveDescriptors(), UpdateNormalAndDepth()
//   Map:          AddMapPoint(pMP), KeyFramesInMap()
//   LocalMapping: isStopped(), stopRequested(), AcceptKeyFrames(), KeyframesInQueue(), InterruptBA()
#pragma once
#include <stddef.h>
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

// what Tracking holds beside the frame (same names as its members)
struct KeyFrameState {
  int mSensor;                        // System::eSensor: MONOCULAR 0, STEREO 1, RGBD 2
  bool mbOnlyTracking;
  unsigned int mnLastRelocFrameId, mnLastKeyFrameId;
  int mMaxFrames, mMinFrames;
  float mThDepth;
};

template <class FrameT>
struct KeyFrameInsertion {
  typedef typename std::remove_pointer<typename decltype(std::declval<FrameT>().mvpMapPoints)::value_type>::type MapPointT;

  struct PointRecord {   // what the call reads of a point a slot holds: stride 16, observed at 12
    float pos[3];
    int32_t observed;
  };

  // the frame as the call takes it; the points a slot or a reference row names, indexed by first sight
  struct Marshal {
    std::map<MapPointT*, int32_t> point_of;
    std::vector<MapPointT*> point;
    std::vector<PointRecord> records;
    std::vector<uint8_t> point_bad, outlier;
    std::vector<int32_t> point_observations, assigned, new_index, ref_slots;
    std::vector<orbfe_map_point> new_points;
    std::vector<float> depth;
    orbfe_unproject_cam cam;
    orbfe_kf_scales scales;
    orbfe_kf_decision_in D;
    orbfe_cov_keyframe row;
    orbfe_kf_header H;
    int32_t n, n_points, n_new, ref_kf;
    orbfe_kf_call C;

    int32_t index_of(MapPointT* pMP) {
      typename std::map<MapPointT*, int32_t>::iterator it = point_of.find(pMP);
      if (it != point_of.end()) return it->second;
      point_of[pMP] = (int32_t)point.size();
      point.push_back(pMP);
      PointRecord r;
      memset(&r, 0, sizeof(r));
      const int n_obs = pMP->Observations();
      r.observed = n_obs > 0 ? 1 : 0;
      records.push_back(r);
      point_bad.push_back(pMP->isBad() ? 1 : 0);
      point_observations.push_back(n_obs);
      return (int32_t)point.size() - 1;
    }

    void frame(FrameT& F, const KeyFrameState& st) {
      static_assert(sizeof(F.mvKeysUn[0]) == sizeof(orbfe_keypoint), "cv::KeyPoint layout");
      memset(&C, 0, sizeof(C));
      memset(&D, 0, sizeof(D));
      memset(&row, 0, sizeof(row));
      memset(&scales, 0, sizeof(scales));
      n = (int32_t)F.N;
      n_new = 0;
      ref_kf = -1;
      assigned.resize((size_t)std::max(n, 1));
      outlier.assign((size_t)std::max(n, 1), 0);
      depth.assign((size_t)std::max(n, 1), 0.0f);
      for (int i = 0; i < n; i++) {
        assigned[i] = F.mvpMapPoints[i] ? index_of(F.mvpMapPoints[i]) : -1;
        outlier[i] = F.mvbOutlier[i] ? 1 : 0;
        depth[i] = F.mvDepth[i];
      }
      const auto Rwc = F.GetRotationInverse();
      const auto Ow = F.GetCameraCenter();
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.Rwc[3 * r + c] = Rwc.template at<float>(r, c);
        cam.Ow[r] = Ow.template at<float>(r);
      }
      cam.cx = FrameT::cx; cam.cy = FrameT::cy; cam.invfx = FrameT::invfx; cam.invfy = FrameT::invfy;
      scales.n_levels = (int32_t)F.mvScaleFactors.size();
      scales.th_depth = st.mThDepth;
      for (size_t l = 0; l < F.mvScaleFactors.size() && l < ORBFE_MAX_LEVELS; l++) scales.scale_factors[l] = F.mvScaleFactors[l];
      D.frame_id = F.mnId;
      D.last_reloc_frame_id = st.mnLastRelocFrameId; D.last_keyframe_id = st.mnLastKeyFrameId;
      D.max_frames = st.mMaxFrames; D.min_frames = st.mMinFrames; D.sensor = st.mSensor; D.only_tracking = st.mbOnlyTracking ? 1 : 0;
      static const orbfe_keypoint no_key = {0, 0, 0, 0, 0, 0, 0};   // a frame without keypoints still hands over arrays
      static const uint8_t no_desc[32] = {0};
      C.keys_un = n > 0 ? reinterpret_cast<const orbfe_keypoint*>(F.mvKeysUn.data()) : &no_key;
      C.desc = n > 0 ? F.mDescriptors.ptr(0) : no_desc;
    }

    // flags and mode chosen, everything marshalled: the one call.  0, or -1 with a line on stderr
    int call(const char* who, int flags, int mode) {
      n_points = (int32_t)point.size();
      const int cap = std::max(n, 1);
      new_points.resize((size_t)cap);
      new_index.resize((size_t)cap);
      if (records.empty()) records.resize(1);
      if (point_bad.empty()) { point_bad.resize(1); point_observations.resize(1); }
      C.depth = depth.data(); C.n = &n; C.cam = &cam; C.assigned = assigned.data(); C.points = records.data(); C.n_points = &n_points;
      C.outlier = outlier.data(); C.decision = &D; C.ref_kf = &ref_kf; C.keyframes = &row; C.point_bad = point_bad.data();
      C.point_observations = point_observations.data(); C.headers = &H; C.new_points = new_points.data(); C.new_index = new_index.data();
      C.n_new = &n_new;
      C.S = 1; C.cap = cap; C.new_cap = cap; C.p_cap = std::max(n_points, 1); C.frame_shift = 0; C.point_stride = (int32_t)sizeof(PointRecord);
      C.observed_offset = (int32_t)offsetof(PointRecord, observed); C.ref_kf_stride = 4; C.n_kf = 1; C.n_map_points = n_points;
      C.mode = mode; C.flags = flags;
      const int rc = orbfe_keyframe_insertion(&C, &scales);
      if (rc != ORBFE_OK) {
        fprintf(stderr, "orbfe_host::%s: orbfe_keyframe_insertion failed: %s (code %d)\n", who, orbfe_last_error(), rc);
        return -1;
      }
      if (H.status != ORBFE_KF_OK) {
        fprintf(stderr, "orbfe_host::%s: the frame was refused\n", who);
        return -1;
      }
      return 0;
    }
  };

  template <class KeyFrameT, class LocalMapperT, class MapT>
  static int NeedNewKeyFrame(FrameT& F, KeyFrameT* pRefKF, LocalMapperT* pLocalMapper, MapT* pMap, const KeyFrameState& st,
                             int* pnMatchesInliers, bool* pbTrackOK) {
    Marshal m;
    m.frame(F, st);
    m.D.mapper_stopped = (pLocalMapper->isStopped() || pLocalMapper->stopRequested()) ? 1 : 0;
    m.D.n_kfs = (int32_t)pMap->KeyFramesInMap();
    m.D.accept_keyframes = pLocalMapper->AcceptKeyFrames() ? 1 : 0;
    m.D.keyframes_in_queue = (int32_t)pLocalMapper->KeyframesInQueue();
    if (pRefKF) {
      for (MapPointT* pMP : pRefKF->GetMapPointMatches()) m.ref_slots.push_back(pMP ? m.index_of(pMP) : -1);
      m.row.n_keys = (int32_t)m.ref_slots.size();
      m.row.slots = (uint64_t)(uintptr_t)m.ref_slots.data();
      m.ref_kf = 0;
    }
    if (m.call("NeedNewKeyFrame", ORBFE_KF_STATISTICS | ORBFE_KF_DECISION, ORBFE_KF_MODE_KEYFRAME)) return -1;
    if (pnMatchesInliers) *pnMatchesInliers = m.H.n_matches_inliers;
    if (pbTrackOK) *pbTrackOK = m.H.track_ok != 0;
    if (m.H.interrupt_ba) pLocalMapper->InterruptBA();   // :951
    return m.H.need;
  }

  // the created entries, in creation order, through `make` (which does what its call site does with entry i)
  template <class Make>
  static int Create(const char* who, FrameT& F, const KeyFrameState& st, int mode, Make make) {
    Marshal m;
    m.frame(F, st);
    if (m.call(who, ORBFE_KF_CREATE, mode)) return -1;
    for (int e = 0; e < m.n_new; e++) make(m.new_index[e]);
    return m.n_new;
  }
};

template <class FrameT, class KeyFrameT, class LocalMapperT, class MapT>
int NeedNewKeyFrame(FrameT& F, KeyFrameT* pRefKF, LocalMapperT* pLocalMapper, MapT* pMap, const KeyFrameState& st, int* pnMatchesInliers = NULL,
                    bool* pbTrackOK = NULL) {
  return KeyFrameInsertion<FrameT>::NeedNewKeyFrame(F, pRefKF, pLocalMapper, pMap, st, pnMatchesInliers, pbTrackOK);
}

template <class FrameT, class KeyFrameT, class MapT>
int CreateNewKeyFramePoints(FrameT& F, KeyFrameT* pKF, MapT* pMap, const KeyFrameState& st) {
  typedef typename KeyFrameInsertion<FrameT>::MapPointT MapPointT;
  if (st.mSensor == ORBFE_KF_SENSOR_MONOCULAR) return 0;   // :973
  return KeyFrameInsertion<FrameT>::Create("CreateNewKeyFramePoints", F, st, ORBFE_KF_MODE_KEYFRAME, [&](int i) {
    F.mvpMapPoints[i] = static_cast<MapPointT*>(NULL);   // :1002 (an empty slot stays empty)
    MapPointT* pNewMP = new MapPointT(F.UnprojectStereo(i), pKF, pMap);
    pNewMP->AddObservation(pKF, i);
    pKF->AddMapPoint(pNewMP, i);
    pNewMP->ComputeDistinctiveDescriptors();
    pNewMP->UpdateNormalAndDepth();
    pMap->AddMapPoint(pNewMP);
    F.mvpMapPoints[i] = pNewMP;
  });
}

template <class FrameT, class MapT, class ListT>
int UpdateLastFramePoints(FrameT& LastFrame, MapT* pMap, ListT& lpTemporalPoints, const KeyFrameState& st) {
  typedef typename KeyFrameInsertion<FrameT>::MapPointT MapPointT;
  return KeyFrameInsertion<FrameT>::Create("UpdateLastFramePoints", LastFrame, st, ORBFE_KF_MODE_LAST_FRAME, [&](int i) {
    MapPointT* pNewMP = new MapPointT(LastFrame.UnprojectStereo(i), pMap, &LastFrame, i);
    LastFrame.mvpMapPoints[i] = pNewMP;
    lpTemporalPoints.push_back(pNewMP);
  });
}

template <class FrameT, class KeyFrameT, class MapT>
int StereoInitializationPoints(FrameT& F, KeyFrameT* pKFini, MapT* pMap, const KeyFrameState& st) {
  typedef typename KeyFrameInsertion<FrameT>::MapPointT MapPointT;
  return KeyFrameInsertion<FrameT>::Create("StereoInitializationPoints", F, st, ORBFE_KF_MODE_STEREO_INIT, [&](int i) {
    MapPointT* pNewMP = new MapPointT(F.UnprojectStereo(i), pKFini, pMap);
    pNewMP->AddObservation(pKFini, i);
    pKFini->AddMapPoint(pNewMP, i);
    pNewMP->ComputeDistinctiveDescriptors();
    pNewMP->UpdateNormalAndDepth();
    pMap->AddMapPoint(pNewMP);
    F.mvpMapPoints[i] = pNewMP;
  });
}

}  // namespace orbfe_host
}  // namespace ORB_SLAM2
