"""The local map of a tracked frame over the C ABI of liborbfe.so (L/ = Source/Libraries/ORB_SLAM2/): the expansion of
Tracking::UpdateLocalKeyFrames behind its vote (L/src/Tracking.cc:1161-1214), Tracking::UpdateLocalPoints (:1090-1113) and the skip flag
Tracking::SearchLocalPoints derives from mnLastFrameSeen (:1036-1049, :1057-1060).

A frame is one VOTES subject of covisibility.py; the call consumes the vote's headers and entries as they are and reads, beside the
vote's tables, one graph row per keyframe row (parent, children, the ten best covisibles).  pack_local_map builds everything from Python
lists; local_map takes host arrays, local_map_device device tensors, and track_local_map_device enqueues vote -> local map ->
SearchLocalPoints on one stream without a host read in between.  All run localmap_kernels.hip; there is no CPU path.
"""
from __future__ import annotations

import numpy as np

from . import _lib, covisibility
from ._lib import (COV_ENTRY_DTYPE, COV_HEADER_DTYPE, COV_SUBJECT_DTYPE, COV_VOTES, LM_BEST, LM_EMPTY, LM_FRAME_DTYPE, LM_GRAPH_DTYPE,
                   LM_HEADER_DTYPE, LM_OK, LM_OVERFLOW, LM_REFUSED, LM_STOP_EXHAUSTED, LM_STOP_PARENT, LM_STOP_SIZE, MAP_POINT_DTYPE)

__all__ = ["LM_GRAPH_DTYPE", "LM_FRAME_DTYPE", "LM_HEADER_DTYPE", "LM_OK", "LM_EMPTY", "LM_OVERFLOW", "LM_REFUSED", "LM_STOP_EXHAUSTED",
           "LM_STOP_SIZE", "LM_STOP_PARENT", "pack_local_map", "pack_seen", "local_map", "local_map_device", "track_local_map_device"]


def pack_local_map(keyframes, points):
    """Python lists -> the tables: what covisibility.pack_covisibility builds (reused as it is) and beside it `graph` (LM_GRAPH_DTYPE,
    one row per keyframe row) and `children` (int32).  A keyframe dict may carry parent (row, or None / -1), children (rows, any
    order: they are stated in ascending `order`, the iteration order of std::set<KeyFrame*>) and best (rows in
    GetVectorCovisibleKeyFrames() order, of which the first ten are kept: GetBestCovisibilityKeyFrames(10))."""
    pack = covisibility.pack_covisibility(keyframes, points)
    order = pack["kf_order"]
    graph = np.zeros(len(keyframes), LM_GRAPH_DTYPE)
    children = []
    for k, kf in enumerate(keyframes):
        parent = kf.get("parent")
        ch = sorted((int(c) for c in kf.get("children", ())), key=lambda c: order[c] if 0 <= c < len(order) else c)
        best = [int(b) for b in kf.get("best", ())][:LM_BEST]
        graph[k]["parent"] = -1 if parent is None else parent
        graph[k]["child_offset"], graph[k]["n_children"], graph[k]["n_best"] = len(children), len(ch), len(best)
        graph[k]["best"][:len(best)] = best
        children += ch
    pack["graph"], pack["children"] = graph, np.asarray(children, np.int32).reshape(-1)
    return pack


def pack_seen(seen):
    """a list with, per frame, the also-seen point indices -> (int32 array, LM_FRAME_DTYPE)"""
    recs = np.zeros(len(seen), LM_FRAME_DTYPE)
    flat, off = [], 0
    for i, s in enumerate(seen):
        a = np.asarray(s, np.int32).reshape(-1)
        recs[i] = (off, len(a))
        flat.append(a)
        off += len(a)
    return (np.concatenate(flat) if flat else np.zeros(0, np.int32)).astype(np.int32), recs


def local_map(pack, votes, conn_cap, subjects, kf_cap, p_cap, seen=None, records=None, out=None):
    """orbfe_local_map on host arrays.  pack: pack_local_map's tables; votes: (COV_HEADER_DTYPE (S), COV_ENTRY_DTYPE (S, conn_cap)) as
    covisibility_counts returned them; subjects: the vote's, a list of (slots, self, mode) or the pair pack_subjects returns; seen: None,
    a list of per-frame index lists or the pair pack_seen returns; records: None or MAP_POINT_DTYPE (n_points), indexed by point.
    Returns a dict: headers LM_HEADER_DTYPE (S), local_kf i32 (S, kf_cap), local_points i32 (S, p_cap), n_points i32 (S) and, with
    records, map_points MAP_POINT_DTYPE (S, p_cap).  Of each list the written head is written (into `out`'s arrays when given, whose
    other bytes stay)."""
    headers, entries = votes
    slots, recs = subjects if isinstance(subjects, tuple) else covisibility.pack_subjects(subjects)
    slots, recs = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(recs, COV_SUBJECT_DTYPE)
    headers, entries = np.ascontiguousarray(headers, COV_HEADER_DTYPE), np.ascontiguousarray(entries, COV_ENTRY_DTYPE)
    S = len(recs)
    if len(headers) != S or entries.size != S * conn_cap:
        raise ValueError("votes: S headers and S x conn_cap entries, one per subject")
    seen_idx, frames = (None, None) if seen is None else seen if isinstance(seen, tuple) else pack_seen(seen)
    if frames is not None:
        seen_idx, frames = np.ascontiguousarray(seen_idx, np.int32), np.ascontiguousarray(frames, LM_FRAME_DTYPE)
        if len(frames) != S:
            raise ValueError("seen: one slice per frame")
    if records is not None:
        records = np.ascontiguousarray(records, MAP_POINT_DTYPE)
        if len(records) != len(pack["point_bad"]):
            raise ValueError("records: one MAP_POINT_DTYPE record per point")
    out = {} if out is None else out
    out.setdefault("headers", np.zeros(S, LM_HEADER_DTYPE))
    out.setdefault("local_kf", np.zeros((S, kf_cap), np.int32))
    out.setdefault("local_points", np.zeros((S, p_cap), np.int32))
    out.setdefault("n_points", np.zeros(S, np.int32))
    if records is not None:
        out.setdefault("map_points", np.zeros((S, p_cap), MAP_POINT_DTYPE))
    want = {"headers": (LM_HEADER_DTYPE, S), "local_kf": (np.int32, S * kf_cap), "local_points": (np.int32, S * p_cap), "n_points": (np.int32, S),
            "map_points": (MAP_POINT_DTYPE, S * p_cap)}
    for name, a in out.items():
        if a.dtype != want[name][0] or a.size != want[name][1] or not a.flags.c_contiguous:
            raise ValueError(f"{name}: a contiguous array of {want[name][1]} {want[name][0]} records")
    _lib.check(_lib.lib().orbfe_local_map(
        _lib.ptr(headers), _lib.ptr(entries), int(conn_cap), _lib.ptr(pack["graph"]), _lib.ptr(pack["children"]), len(pack["children"]),
        _lib.ptr(pack["table"]), _lib.ptr(pack["kf_bad"]), len(pack["table"]), _lib.ptr(pack["point_bad"]), len(pack["point_bad"]),
        _lib.ptr(slots), len(slots), _lib.ptr(recs), _lib.ptr(frames), _lib.ptr(seen_idx), 0 if seen_idx is None else len(seen_idx),
        _lib.ptr(records), S, int(kf_cap), int(p_cap), _lib.ptr(out["headers"]), _lib.ptr(out["local_kf"]), _lib.ptr(out["local_points"]),
        _lib.ptr(out["n_points"]), _lib.ptr(out.get("map_points"))), "orbfe_local_map")
    return out


def local_map_device(headers, entries, conn_cap, graph, children, table, kf_bad, point_bad, slots, subjects, frames, seen, records, kf_cap,
                     p_cap, lm_headers, local_kf, local_points, n_points, map_points, stream=None):
    """orbfe_local_map_batch_device on torch CUDA tensors: headers (S, 32) u8 and entries (S * conn_cap, 8) u8 as
    covisibility_counts_device left them, graph (n_kf, 56) u8 = LM_GRAPH_DTYPE, children i32, table (n_kf, 48) u8 = COV_KEYFRAME_DTYPE
    with DEVICE addresses, kf_bad (n_kf) u8, point_bad (P) u8, slots i32 and subjects (S, 16) u8 of the vote, frames (S, 8) u8 =
    LM_FRAME_DTYPE and seen i32 (both None: no frame has also-seen points), records (P, 72) u8 = MAP_POINT_DTYPE or None; outputs
    lm_headers (S, 32) u8, local_kf (S, kf_cap) i32, local_points (S, p_cap) i32, n_points (S) i32, map_points (S, p_cap, 72) u8 (None
    without records).  Asynchronous on stream (a torch.cuda.Stream, or None for the NULL stream)."""
    _lib.check(_lib.lib().orbfe_local_map_batch_device(
        int(subjects.shape[0]), _lib.ptr(headers), _lib.ptr(entries), int(conn_cap), _lib.ptr(graph), _lib.ptr(children), int(children.shape[0]),
        _lib.ptr(table), _lib.ptr(kf_bad), int(table.shape[0]), _lib.ptr(point_bad), int(point_bad.shape[0]), _lib.ptr(slots),
        int(slots.shape[0]), _lib.ptr(subjects), _lib.ptr(frames), _lib.ptr(seen), 0 if seen is None else int(seen.shape[0]), _lib.ptr(records),
        int(kf_cap), int(p_cap), _lib.ptr(lm_headers), _lib.ptr(local_kf), _lib.ptr(local_points), _lib.ptr(n_points), _lib.ptr(map_points),
        _lib.stream_handle(stream)), "orbfe_local_map_batch_device")


def track_local_map_device(matcher, stream, map_tables, slots, subjects, frames, seen, conn_cap, kf_cap, vote_headers, vote_entries,
                           lm_headers, local_kf, local_points, n_points, map_points, kps, desc, n, u_right, bounds, frustums, th, nnratio,
                           track, blocked, assigned, n_to_match, n_matches):
    """The body of Tracking::TrackLocalMap between the pose and its optimisation for a chunk of frames, enqueued on ONE stream (a
    torch.cuda.Stream) with no host read in between: the vote (covisibility_counts_device), the local map (local_map_device) and
    Tracking::SearchLocalPoints (Matcher.search_local_points_batch).  map_tables: a dict of resident tensors obs, recs, point_bad,
    kf_order, kf_bad, graph, children, table and records (see the two calls); every other argument is the tensor of that name in
    them; p_cap is map_points.shape[1].  A frame whose vote is EMPTY keeps what n_points and map_points held before the call."""
    t = map_tables
    covisibility.covisibility_counts_device(t["obs"], t["recs"], t["point_bad"], t["kf_order"], t["kf_bad"], slots, subjects, conn_cap,
                                            vote_headers, vote_entries, stream=stream)
    local_map_device(vote_headers, vote_entries, conn_cap, t["graph"], t["children"], t["table"], t["kf_bad"], t["point_bad"], slots, subjects,
                     frames, seen, t["records"], kf_cap, map_points.shape[1], lm_headers, local_kf, local_points, n_points, map_points,
                     stream=stream)
    matcher.search_local_points_batch(kps, desc, n, u_right, bounds, frustums, map_points, n_points, th, nnratio, track, blocked, assigned,
                                      n_to_match, n_matches, stream=stream)
