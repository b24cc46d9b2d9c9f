"""LocalMapping::CreateNewMapPoints over the C ABI of liborbfe.so (L/src/LocalMapping.cc:185-423, L/ = Source/Libraries/ORB_SLAM2/):
new map points from the matches of a keyframe with its covisible neighbours.

triangulate_matches is the geometry of one (pKF1, pKF2) pair on host arrays, triangulate_matches_batch the same for K neighbours in
one launch on device tensors, create_new_map_points the whole loop: per neighbour the baseline gate, SearchForTriangulation and the
triangulation back to back on the device, pKF1 staged once, its "has a map point" mask kept on the device between neighbours.  All
three run mapping_kernels.hip; there is no CPU path.

search_in_neighbors is LocalMapping::SearchInNeighbors (:425-509) from the target list on, over an index-based map: all Fuse calls of
the forward loop as one batched search of a matcher.FuseBatch (fuse_kernels.hip), replayed in target order with the rows of changed
descriptors searched again.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import EPIPOLAR_DTYPE, KP_DTYPE, NEW_POINT_DTYPE, TRI_NEIGHBOR_DTYPE, TRI_VIEW_DTYPE
from .matcher import featvec_arrays

__all__ = ["TRI_VIEW_DTYPE", "NEW_POINT_DTYPE", "tri_view", "triangulate_matches", "triangulate_matches_batch", "create_new_map_points",
           "search_in_neighbors", "DeviceFuseSearch"]


def tri_view(Rcw, tcw, fx, fy, cx, cy, mb, scale_factors, level_sigma2, Ow=None) -> np.ndarray:
    """One orbfe_tri_view record.  Rcw 3 x 3, tcw 3; Ow defaults to -Rcw^T tcw; invfx = 1 / fx and mbf = mb * fx in float, as the
    KeyFrame holds them; n_levels is the length of scale_factors."""
    sf = np.asarray(scale_factors, np.float32).reshape(-1)
    sg = np.asarray(level_sigma2, np.float32).reshape(-1)
    v = np.zeros(1, TRI_VIEW_DTYPE)
    R = np.asarray(Rcw, np.float32).reshape(3, 3)
    t = np.asarray(tcw, np.float32).reshape(3)
    v["Rcw"][0], v["tcw"][0] = R.reshape(9), t
    v["Ow"][0] = -(R.T @ t) if Ow is None else np.asarray(Ow, np.float32).reshape(3)
    v["fx"], v["fy"], v["cx"], v["cy"], v["mb"] = fx, fy, cx, cy, mb
    v["invfx"], v["invfy"] = np.float32(1) / np.float32(fx), np.float32(1) / np.float32(fy)
    v["mbf"] = np.float32(mb) * np.float32(fx)
    v["n_levels"] = len(sf)
    v["scale_factors"][0, :min(len(sf), _lib.MAX_LEVELS)] = sf[:_lib.MAX_LEVELS]
    v["level_sigma2"][0, :min(len(sg), _lib.MAX_LEVELS)] = sg[:_lib.MAX_LEVELS]
    return v


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def triangulate_matches(view1, keys1, u_right1, depth1, view2, keys2, u_right2, depth2, matchA):
    """The loop body of CreateNewMapPoints for every match of one pair.  view*: tri_view(...); keys*: KP_DTYPE = mvKeysUn; u_right* /
    depth*: float32 = mvuRight / mvDepth, or both None (monocular); matchA: (nA) int32 from search_for_triangulation.  Returns
    (points, n_new): NEW_POINT_DTYPE (nA) and the number of accepted rows."""
    keys1, keys2 = np.ascontiguousarray(keys1, KP_DTYPE), np.ascontiguousarray(keys2, KP_DTYPE)
    v1, v2 = np.ascontiguousarray(view1, TRI_VIEW_DTYPE).reshape(1), np.ascontiguousarray(view2, TRI_VIEW_DTYPE).reshape(1)
    ur1, z1, ur2, z2 = _f32(u_right1), _f32(depth1), _f32(u_right2), _f32(depth2)
    matchA = np.ascontiguousarray(matchA, np.int32)
    nA, nB = len(keys1), len(keys2)
    if len(matchA) != nA or any(a is not None and len(a) != n for a, n in ((ur1, nA), (z1, nA), (ur2, nB), (z2, nB))):
        raise ValueError("matchA, u_right1 and depth1 have one entry per pKF1 keypoint, u_right2 and depth2 one per pKF2 keypoint")
    out = np.zeros(nA, NEW_POINT_DTYPE)
    n_new = C.c_int(0)
    _lib.check(_lib.lib().orbfe_triangulate_matches(_lib.ptr(v1), _lib.ptr(keys1), _lib.ptr(ur1), _lib.ptr(z1), nA, _lib.ptr(v2),
                                                    _lib.ptr(keys2), _lib.ptr(ur2), _lib.ptr(z2), nB, _lib.ptr(matchA), _lib.ptr(out),
                                                    C.byref(n_new)), "orbfe_triangulate_matches")
    return out, n_new.value


def triangulate_matches_batch(view1, keys1, u_right1, depth1, nA, view2, keys2, u_right2, depth2, nB, matchA, out, n_new, stream=None):
    """orbfe_triangulate_matches_batch_device on torch CUDA tensors: view1 (224) u8 = one TRI_VIEW_DTYPE record, keys1 (capA,28) u8,
    u_right1 / depth1 (capA) f32 or None, nA (K) i32, view2 (K,224) u8, keys2 (K,capB,28) u8, u_right2 / depth2 (K,capB) f32 or None,
    nB (K) i32, matchA (K,capA) i32, out (K,capA,44) u8 = NEW_POINT_DTYPE, n_new (K) i32.  stream: a torch.cuda.Stream, or None for
    the NULL stream."""
    K, capA, capB = int(matchA.shape[0]), int(matchA.shape[1]), int(keys2.shape[1])
    _lib.check(_lib.lib().orbfe_triangulate_matches_batch_device(K, _lib.ptr(view1), _lib.ptr(keys1), _lib.ptr(u_right1), _lib.ptr(depth1),
                                                                 _lib.ptr(nA), capA, _lib.ptr(view2), _lib.ptr(keys2), _lib.ptr(u_right2),
                                                                 _lib.ptr(depth2), _lib.ptr(nB), capB, _lib.ptr(matchA), _lib.ptr(out),
                                                                 _lib.ptr(n_new), _lib.stream_handle(stream)),
               "orbfe_triangulate_matches_batch_device")


def create_new_map_points(keysA, descA, u_rightA, depthA, has_mpA, groupsA, viewA, neighbors, monocular=False, only_stereo=False,
                          check_orientation=True):
    """The neighbour loop of CreateNewMapPoints for pKF1 = A.  groupsA: pKF1->mFeatVec as {node_id: [feature indices]}; neighbors: a
    list of dicts with keys, desc, u_right, depth (None: monocular), has_mp, groups, view (tri_view), epipolar (EPIPOLAR_DTYPE) and,
    for monocular=True, median_depth.  Returns (points, n_matches, n_new, has_mp): NEW_POINT_DTYPE (K, nA), int32 (K) (-1 for a
    neighbour the baseline gate skipped), int32 (K), and has_mpA with the accepted features set."""
    keysA = np.ascontiguousarray(keysA, KP_DTYPE)
    descA = np.ascontiguousarray(descA, np.uint8).reshape(-1, 32)
    urA, zA = _f32(u_rightA), _f32(depthA)
    has = np.ascontiguousarray(has_mpA, np.uint8).copy()
    vA = np.ascontiguousarray(viewA, TRI_VIEW_DTYPE).reshape(1)
    nodesA, nnA, idxA = featvec_arrays(groupsA)
    nA, K = len(keysA), len(neighbors)
    rec = np.zeros(max(K, 1), TRI_NEIGHBOR_DTYPE)
    keep = [nodesA, idxA]
    for k, nb in enumerate(neighbors):
        keys = np.ascontiguousarray(nb["keys"], KP_DTYPE)
        desc = np.ascontiguousarray(nb["desc"], np.uint8).reshape(-1, 32)
        ur, z = _f32(nb.get("u_right")), _f32(nb.get("depth"))
        hm = np.ascontiguousarray(nb["has_mp"], np.uint8)
        nodes, nn, idx = featvec_arrays(nb["groups"])
        keep += [keys, desc, ur, z, hm, nodes, idx]
        r = rec[k]
        r["keys"], r["desc"], r["has_mp"] = keys.ctypes.data, desc.ctypes.data, hm.ctypes.data
        r["u_right"] = 0 if ur is None else ur.ctypes.data
        r["depth"] = 0 if z is None else z.ctypes.data
        r["nodes"], r["idx"] = C.cast(nodes, C.c_void_p).value or 0, idx.ctypes.data
        r["n"], r["n_nodes"] = len(keys), nn
        r["view"] = np.ascontiguousarray(nb["view"], TRI_VIEW_DTYPE).reshape(1)[0]
        r["ep"] = np.ascontiguousarray(nb["epipolar"], EPIPOLAR_DTYPE).reshape(1)[0]
        r["median_depth"] = nb.get("median_depth", 0.0)
    points = np.zeros((K, nA), NEW_POINT_DTYPE)
    n_matches, n_new = np.zeros(K, np.int32), np.zeros(K, np.int32)
    _lib.check(_lib.lib().orbfe_create_new_map_points(_lib.ptr(keysA), _lib.ptr(descA), _lib.ptr(urA), _lib.ptr(zA), _lib.ptr(has), nA,
                                                      C.cast(nodesA, C.c_void_p), nnA, _lib.ptr(idxA), _lib.ptr(vA), _lib.ptr(rec), K,
                                                      int(monocular), int(only_stereo), int(check_orientation), _lib.ptr(points),
                                                      _lib.ptr(n_matches), _lib.ptr(n_new)), "orbfe_create_new_map_points")
    del keep
    return points, n_matches, n_new, has


# ---- LocalMapping::SearchInNeighbors (L/src/LocalMapping.cc:425-509): every Fuse call of a keyframe batched ------------------------------
class DeviceFuseSearch:
    """The row-search backend of search_in_neighbors on the device: a matcher.FuseBatch over the targets of `map`."""

    def __init__(self, map, targets, th):
        from .matcher import FrameView, FuseBatch
        views, cams, inv = [], [], []
        for kf in targets:
            t = map.target(kf, th)
            views.append(FrameView(t["keys"], t["desc"], *t["bounds"], u_right=t["u_right"]))
            cams.append(np.ascontiguousarray(t["camera"], _lib.KF_CAMERA_DTYPE).reshape(-1)[0])
            inv.append(t["inv_level_sigma2"])
        self.batch = FuseBatch(views, np.array(cams, _lib.KF_CAMERA_DTYPE), inv, _lib.KF_FUSE)
        self.rows = None

    def search(self, points, point_idx=None, first_target=0, skip=None):
        self.rows = self.batch.search(points, point_idx, first_target, skip, results=self.rows)
        return self.rows

    def close(self):
        self.batch.close()


def _fuse_records(map, ids):
    """KF_POINT_DTYPE records of the points `ids` (-1 = NULL); a NULL or bad point is a skipped record"""
    rec = np.zeros(len(ids), _lib.KF_POINT_DTYPE)
    for j, p in enumerate(ids):
        if p < 0 or map.is_bad(p):
            rec[j]["skip"] = 1
        else:
            map.fill_point(p, rec[j])
    return rec


def _fuse_skip_mask(map, ids, targets):
    """(K, n) bytes: the rows ORBmatcher::Fuse skips at :787 as the map stands (NULL, isBad(), IsInKeyFrame(target))"""
    m = np.zeros((len(targets), len(ids)), np.uint8)
    for j, p in enumerate(ids):
        if p < 0 or map.is_bad(p):
            m[:, j] = 1
        else:
            for k, kf in enumerate(targets):
                m[k, j] = map.in_keyframe(p, kf)
    return m


def _fuse_update(map, kf, ids, rows, log, th_low=50):
    """The map update of ORBmatcher::Fuse (L/src/ORBmatcher.cc:870-884) for one target, in point order on the live map, from the
    target's rows of the batch; the two tests of :787 are taken again on the live objects.  Returns nFused."""
    n_fused = 0
    for i, p in enumerate(ids):
        if p < 0 or map.is_bad(p) or map.in_keyframe(p, kf):
            continue
        best_idx, best_dist = int(rows[i]["best_idx"]), int(rows[i]["best_dist"])
        if best_idx < 0 or best_dist > th_low:
            continue
        in_kf = map.map_point(kf, best_idx)
        if in_kf >= 0:
            if not map.is_bad(in_kf):
                if map.observations(in_kf) > map.observations(p):
                    log.append(("replace", p, in_kf))
                    map.replace(p, in_kf)
                else:
                    log.append(("replace", in_kf, p))
                    map.replace(in_kf, p)
            else:
                log.append(("bad", p, kf, best_idx))
        else:
            log.append(("add", p, kf, best_idx))
            map.add_observation(p, kf, best_idx)
            map.add_map_point(kf, p, best_idx)
        n_fused += 1
    return n_fused


def search_in_neighbors(map, current, targets, th=3.0, search=None):
    """LocalMapping::SearchInNeighbors from the target list on (L/src/LocalMapping.cc:457-509) with all Fuse calls of the forward loop
    in one batched search.  The K calls of the reference depend on each other only through the map, and the one search input a
    Replace changes is the survivor's descriptor: so every row (target k, point i) is searched once with the descriptors as they
    are, the targets are replayed in order on the live map, and before the replay enters target k + 1 the points whose descriptor
    bytes differ from those their rows were computed with are searched again in the targets k + 1 .. K-1 (one partial search per
    boundary at most).  The reverse pass (:469-493) is one Fuse into `current` with the candidates collected from the live map.

    `map` is duck-typed and index-based (keyframes and points are ints, -1 = none):
      point_matches(kf) -> ids, GetMapPointMatches()      map_point(kf, idx)           is_bad(p)          in_keyframe(p, kf)
      observations(p) -> MapPoint::Observations()          replace(p, q): p->Replace(q)  add_observation(p, kf, idx)
      add_map_point(kf, p, idx)                            descriptor(p) -> 32 bytes     fill_point(p, record)
      target(kf, th) -> dict(keys, desc, u_right, bounds, camera, inv_level_sigma2)
      optional: update_points(kf) (:495-505) and update_connections(kf) (:508)
    point_matches(current) must hold no point twice.  `search(map, targets, th)` makes the row-search backend (search / close;
    default DeviceFuseSearch; a backend with a true `no_repair` attribute skips the repair searches, for tests).
    Returns dict(log, n_fused, n_full, n_repair): the operations in order -- ("add", p, kf, idx), ("replace", dying, survivor),
    ("bad", p, kf, idx) -- the sum of the Fuse return values and the number of full and of repair searches made."""
    make = DeviceFuseSearch if search is None else search
    log, n_fused, n_full, n_repair = [], 0, 0, 0
    ids = [int(p) for p in map.point_matches(current)]
    live = [p for p in ids if p >= 0]
    if len(set(live)) != len(live):
        raise ValueError("point_matches(current) holds a point twice")
    if targets and ids:
        backend = make(map, targets, th)
        try:
            rec = _fuse_records(map, ids)
            rows = backend.search(rec, None, 0, _fuse_skip_mask(map, ids, targets))
            n_full += 1
            for k, kf in enumerate(targets):
                if k > 0 and not getattr(backend, "no_repair", False):
                    stale = [i for i, p in enumerate(ids) if p >= 0 and not map.is_bad(p) and
                             bytes(np.asarray(map.descriptor(p), np.uint8)) != bytes(rec[i]["desc"])]
                    if stale:
                        rec[stale] = _fuse_records(map, [ids[i] for i in stale])
                        rows = backend.search(rec[stale], np.array(stale, np.int32), k, None)
                        n_repair += 1
                log.append(("target", kf))
                n_fused += _fuse_update(map, kf, ids, rows[k], log)
        finally:
            backend.close()
    # the candidates of the reverse pass, from the live map: every point of a target once (mnFuseCandidateForKF)
    cand, seen = [], set()
    for kf in targets:
        for p in map.point_matches(kf):
            p = int(p)
            if p < 0 or map.is_bad(p) or p in seen:
                continue
            seen.add(p)
            cand.append(p)
    log.append(("target", current))
    if cand:
        backend = make(map, [current], th)
        try:
            rows = backend.search(_fuse_records(map, cand), None, 0, _fuse_skip_mask(map, cand, [current]))
            n_full += 1
            n_fused += _fuse_update(map, current, cand, rows[0], log)
        finally:
            backend.close()
    if hasattr(map, "update_points"):
        map.update_points(current)
    if hasattr(map, "update_connections"):
        map.update_connections(current)
    return dict(log=log, n_fused=n_fused, n_full=n_full, n_repair=n_repair)
