"""The covisibility graph over the C ABI of liborbfe.so (L/ = Source/Libraries/ORB_SLAM2/): the counts of KeyFrame::UpdateConnections
(L/src/KeyFrame.cc:268-354) and of the vote of Tracking::UpdateLocalKeyFrames (L/src/Tracking.cc:1115-1159), and
LocalMapping::KeyFrameCulling (L/src/LocalMapping.cc:595-655) with its sequential side effects.

Both read the tables of map_point.py -- the observation array and, per point, its slice of it -- plus a bad byte per point and, per
keyframe ROW, its position `order` in the iteration order of the reference's std::map<KeyFrame*, ...>, which the caller states.
pack_covisibility builds the tables from Python lists; covisibility_counts and cull_keyframes take them on host arrays,
covisibility_counts_device and cull_keyframes_device on device tensors.  All four run covis_kernels.hip; there is no CPU path.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import (COV_CONNECTIONS, COV_CULLED, COV_EMPTY, COV_ENTRY_DTYPE, COV_HEADER_DTYPE, COV_IS_ID0, COV_KEPT, COV_KEYFRAME_DTYPE,
                   COV_MARKED, COV_NOT_ERASE, COV_OK, COV_OVERFLOW, COV_PROBLEM_DTYPE, COV_REFUSED, COV_ROW_REFUSED, COV_SKIPPED_ID0,
                   COV_SUBJECT_DTYPE, COV_VERDICT_DTYPE, COV_VOTES, KP_DTYPE, MP_OBS_DTYPE, MP_POINT_DTYPE)

__all__ = ["COV_SUBJECT_DTYPE", "COV_HEADER_DTYPE", "COV_ENTRY_DTYPE", "COV_KEYFRAME_DTYPE", "COV_PROBLEM_DTYPE", "COV_VERDICT_DTYPE",
           "COV_CONNECTIONS", "COV_VOTES", "COV_OK", "COV_EMPTY", "COV_OVERFLOW", "COV_REFUSED", "COV_KEPT", "COV_CULLED", "COV_MARKED",
           "COV_SKIPPED_ID0", "COV_ROW_REFUSED", "COV_IS_ID0", "COV_NOT_ERASE", "pack_covisibility", "pack_subjects", "pack_problems",
           "covisibility_counts", "covisibility_counts_device", "cull_keyframes", "cull_keyframes_device"]


def pack_covisibility(keyframes, points):
    """Python lists -> the tables.  keyframes: a list of dicts with order, bad, and for culling slots (point index or -1 per keypoint =
    mvpMapPoints), octaves (mvKeysUn[i].octave), u_right and depth (mvuRight, mvDepth; None: absent), th_depth, id0, not_erase; points: a
    list of dicts with obs (a list of (keyframe row, keypoint index) in map order; empty for a bad point), bad and n_obs_weighted
    (Observations()).  Returns a dict: obs MP_OBS_DTYPE, recs MP_POINT_DTYPE, point_bad u8, n_obs_weighted i32, kf_order i32, kf_bad u8,
    table COV_KEYFRAME_DTYPE with HOST addresses, and keys / u_right / depth / slots, the per-keyframe arrays those addresses point into."""
    n_kf = len(keyframes)
    table = np.zeros(n_kf, COV_KEYFRAME_DTYPE)
    order, kf_bad = np.zeros(n_kf, np.int32), np.zeros(n_kf, np.uint8)
    keys, right, depth, slots = [], [], [], []
    for k, kf in enumerate(keyframes):
        order[k], kf_bad[k] = kf.get("order", k), int(bool(kf.get("bad", False)))
        s = np.ascontiguousarray(kf.get("slots", ()), np.int32).reshape(-1)
        kp = np.zeros(len(s), KP_DTYPE)
        kp["octave"] = np.asarray(kf.get("octaves", np.zeros(len(s))), np.int32)
        r = None if kf.get("u_right") is None else np.ascontiguousarray(kf["u_right"], np.float32).reshape(len(s))
        d = None if kf.get("depth") is None else np.ascontiguousarray(kf["depth"], np.float32).reshape(len(s))
        keys.append(kp), right.append(r), depth.append(d), slots.append(s)
        table[k]["n_keys"], table[k]["th_depth"] = len(s), kf.get("th_depth", 0.0)
        table[k]["flags"] = (COV_IS_ID0 if kf.get("id0") else 0) | (COV_NOT_ERASE if kf.get("not_erase") else 0)
        if len(s):
            table[k]["keys_un"], table[k]["slots"] = kp.ctypes.data, s.ctypes.data
            table[k]["u_right"] = 0 if r is None else r.ctypes.data
            table[k]["depth"] = 0 if d is None else d.ctypes.data
    n_total = sum(len(p["obs"]) for p in points)
    obs, recs = np.zeros(n_total, MP_OBS_DTYPE), np.zeros(len(points), MP_POINT_DTYPE)
    point_bad, weighted = np.zeros(len(points), np.uint8), np.zeros(len(points), np.int32)
    off = 0
    for i, p in enumerate(points):
        n = len(p["obs"])
        if n:
            o = np.asarray(p["obs"], np.int32).reshape(n, 2)
            obs["kf"][off:off + n], obs["idx"][off:off + n] = o[:, 0], o[:, 1]
        recs[i]["obs_offset"], recs[i]["n_obs"] = off, n
        point_bad[i], weighted[i] = int(bool(p.get("bad", False))), p.get("n_obs_weighted", n)
        off += n
    return {"obs": obs, "recs": recs, "point_bad": point_bad, "n_obs_weighted": weighted, "kf_order": order, "kf_bad": kf_bad, "table": table,
            "keys": keys, "u_right": right, "depth": depth, "slots": slots}


def pack_subjects(subjects):
    """a list of (slots, self, mode) -> (slot array int32, COV_SUBJECT_DTYPE)"""
    recs = np.zeros(len(subjects), COV_SUBJECT_DTYPE)
    flat, off = [], 0
    for i, (slots, me, mode) in enumerate(subjects):
        s = np.asarray(slots, np.int32).reshape(-1)
        recs[i] = (off, len(s), me, mode)
        flat.append(s)
        off += len(s)
    return (np.concatenate(flat) if flat else np.zeros(0, np.int32)).astype(np.int32), recs


def pack_problems(problems):
    """a list of (local keyframe rows, monocular) -> (local array int32, COV_PROBLEM_DTYPE)"""
    recs = np.zeros(len(problems), COV_PROBLEM_DTYPE)
    flat, off = [], 0
    for i, (rows, mono) in enumerate(problems):
        r = np.asarray(rows, np.int32).reshape(-1)
        recs[i] = (off, len(r), int(bool(mono)), 0)
        flat.append(r)
        off += len(r)
    return (np.concatenate(flat) if flat else np.zeros(0, np.int32)).astype(np.int32), recs


def covisibility_counts(pack, subjects, conn_cap, headers=None, entries=None):
    """orbfe_covis_count on host arrays.  pack: pack_covisibility's tables; subjects: a list of (slots, self, mode) or the pair
    pack_subjects returns.  Returns (COV_HEADER_DTYPE (S), COV_ENTRY_DTYPE (S, conn_cap)); of a subject's entries the first n_written
    are written (into `entries` when given, whose other bytes stay)."""
    slots, recs = subjects if isinstance(subjects, tuple) else pack_subjects(subjects)
    slots, recs = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(recs, COV_SUBJECT_DTYPE)
    S = len(recs)
    headers = np.zeros(S, COV_HEADER_DTYPE) if headers is None else headers
    entries = np.zeros((S, conn_cap), COV_ENTRY_DTYPE) if entries is None else entries
    if headers.dtype != COV_HEADER_DTYPE or len(headers) != S or entries.dtype != COV_ENTRY_DTYPE or entries.size != S * conn_cap or \
            not (headers.flags.c_contiguous and entries.flags.c_contiguous):
        raise ValueError("headers: S contiguous COV_HEADER_DTYPE records; entries: S x conn_cap contiguous COV_ENTRY_DTYPE records")
    _lib.check(_lib.lib().orbfe_covis_count(_lib.ptr(pack["obs"]), len(pack["obs"]), _lib.ptr(pack["recs"]), _lib.ptr(pack["point_bad"]),
                                            len(pack["recs"]), _lib.ptr(pack["kf_order"]), _lib.ptr(pack["kf_bad"]), len(pack["kf_order"]),
                                            _lib.ptr(slots), len(slots), _lib.ptr(recs), S, int(conn_cap), _lib.ptr(headers),
                                            _lib.ptr(entries)), "orbfe_covis_count")
    return headers, entries


def covisibility_counts_device(obs, recs, point_bad, kf_order, kf_bad, slots, subjects, conn_cap, headers, entries, stream=None):
    """orbfe_covis_count_batch_device on torch CUDA tensors: obs (n_obs_total, 8) u8 = MP_OBS_DTYPE, recs (P, 16) u8 = MP_POINT_DTYPE,
    point_bad (P) u8, kf_order (n_kf) i32, kf_bad (n_kf) u8, slots (n_slots_total) i32, subjects (S, 16) u8 = COV_SUBJECT_DTYPE, headers
    (S, 32) u8, entries (S * conn_cap, 8) u8.  Asynchronous on stream (a torch.cuda.Stream, or None for the NULL stream)."""
    _lib.check(_lib.lib().orbfe_covis_count_batch_device(int(subjects.shape[0]), _lib.ptr(obs), int(obs.shape[0]), _lib.ptr(recs),
                                                         _lib.ptr(point_bad), int(recs.shape[0]), _lib.ptr(kf_order), _lib.ptr(kf_bad),
                                                         int(kf_order.shape[0]), _lib.ptr(slots), int(slots.shape[0]), _lib.ptr(subjects),
                                                         int(conn_cap), _lib.ptr(headers), _lib.ptr(entries), _lib.stream_handle(stream)),
               "orbfe_covis_count_batch_device")


def cull_keyframes(pack, problems, verdicts=None):
    """orbfe_covis_cull_keyframes on host arrays.  problems: a list of (local keyframe rows in GetVectorCovisibleKeyFrames() order,
    monocular) or the pair pack_problems returns.  Returns COV_VERDICT_DTYPE, one record per element of the local array."""
    local, recs = problems if isinstance(problems, tuple) else pack_problems(problems)
    local, recs = np.ascontiguousarray(local, np.int32), np.ascontiguousarray(recs, COV_PROBLEM_DTYPE)
    verdicts = np.zeros(len(local), COV_VERDICT_DTYPE) if verdicts is None else verdicts
    if verdicts.dtype != COV_VERDICT_DTYPE or len(verdicts) != len(local) or not verdicts.flags.c_contiguous:
        raise ValueError("verdicts: a contiguous COV_VERDICT_DTYPE array with one record per local keyframe")
    _lib.check(_lib.lib().orbfe_covis_cull_keyframes(_lib.ptr(pack["obs"]), len(pack["obs"]), _lib.ptr(pack["recs"]), _lib.ptr(pack["point_bad"]),
                                                     _lib.ptr(pack["n_obs_weighted"]), len(pack["recs"]), _lib.ptr(pack["table"]),
                                                     len(pack["table"]), _lib.ptr(local), len(local), _lib.ptr(recs), len(recs),
                                                     _lib.ptr(verdicts)), "orbfe_covis_cull_keyframes")
    return verdicts


def cull_keyframes_device(obs, recs, point_bad, n_obs_weighted, table, local, problems, verdicts, stream=None):
    """orbfe_covis_cull_keyframes_batch_device on torch CUDA tensors: as covisibility_counts_device, with n_obs_weighted (P) i32, table
    (n_kf, 48) u8 = COV_KEYFRAME_DTYPE with DEVICE addresses, local (n_local_total) i32, problems (Q, 16) u8 = COV_PROBLEM_DTYPE and
    verdicts (n_local_total, 16) u8.  Asynchronous on stream."""
    _lib.check(_lib.lib().orbfe_covis_cull_keyframes_batch_device(int(problems.shape[0]), _lib.ptr(obs), int(obs.shape[0]), _lib.ptr(recs),
                                                                  _lib.ptr(point_bad), _lib.ptr(n_obs_weighted), int(recs.shape[0]),
                                                                  _lib.ptr(table), int(table.shape[0]), _lib.ptr(local), int(local.shape[0]),
                                                                  _lib.ptr(problems), _lib.ptr(verdicts), _lib.stream_handle(stream)),
               "orbfe_covis_cull_keyframes_batch_device")
