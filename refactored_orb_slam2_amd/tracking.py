"""The keyframe decision and the close stereo points of a tracked frame over the C ABI of liborbfe.so (L/ =
Source/Libraries/ORB_SLAM2/): the statistics tail of Tracking::TrackLocalMap (L/src/Tracking.cc:851-877), Tracking::NeedNewKeyFrame
(:880-962), the depth-ordered point creation of Tracking::CreateNewKeyFrame (:973-1024), the temporal points of
Tracking::UpdateLastFrame (:732-777) and the points of Tracking::StereoInitialization (:455-479).

keyframe_insertion takes a batch of frames as host arrays, keyframe_insertion_device as device tensors (asynchronous, one launch);
need_new_keyframe, create_new_keyframe, update_last_frame_points and stereo_initialization are the four call sites on one frame,
their *_batch forms on a batch, and pack_decision / pack_scales / pack_reference build the records.  All run keyframe_kernels.hip;
there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (COV_KEYFRAME_DTYPE, KF_C1A, KF_C1B, KF_C1C, KF_C2, KF_CREATE, KF_DECISION, KF_DECISION_DTYPE, KF_HEADER_DTYPE,
                   KF_MODE_KEYFRAME, KF_MODE_LAST_FRAME, KF_MODE_STEREO_INIT, KF_OK, KF_OVERFLOW, KF_REFUSED, KF_SCALES_DTYPE,
                   KF_SENSOR_MONOCULAR, KF_SENSOR_RGBD, KF_SENSOR_STEREO, KF_STATISTICS, KP_DTYPE, MAP_POINT_DTYPE, UNPROJECT_CAM_DTYPE)

__all__ = ["KF_DECISION_DTYPE", "KF_SCALES_DTYPE", "KF_HEADER_DTYPE", "KF_STATISTICS", "KF_DECISION", "KF_CREATE", "KF_MODE_KEYFRAME",
           "KF_MODE_LAST_FRAME", "KF_MODE_STEREO_INIT", "KF_SENSOR_MONOCULAR", "KF_SENSOR_STEREO", "KF_SENSOR_RGBD", "KF_OK", "KF_OVERFLOW",
           "KF_REFUSED", "KF_C1A", "KF_C1B", "KF_C1C", "KF_C2", "OBSERVED_OFFSET", "pack_decision", "pack_scales", "pack_reference",
           "keyframe_insertion", "keyframe_insertion_device", "need_new_keyframe", "need_new_keyframe_batch", "create_new_keyframe",
           "create_new_keyframe_batch", "update_last_frame_points", "update_last_frame_points_batch", "stereo_initialization",
           "stereo_initialization_batch"]

OBSERVED_OFFSET = MAP_POINT_DTYPE.fields["observed"][1]   # of orbfe_map_point: 36


def pack_decision(frames):
    """a list of dicts (frame_id, last_reloc_frame_id, last_keyframe_id, max_frames, min_frames, sensor, only_tracking,
    mapper_stopped, accept_keyframes, keyframes_in_queue, n_kfs; what is missing is 0) -> KF_DECISION_DTYPE (S)"""
    rec = np.zeros(len(frames), KF_DECISION_DTYPE)
    for f, d in enumerate(frames):
        for k, v in d.items():
            rec[f][k] = v
    return rec


def pack_scales(scale_factors, th_depth):
    """mvScaleFactors and mThDepth -> one KF_SCALES_DTYPE record"""
    sf = np.asarray(scale_factors, np.float32).reshape(-1)
    rec = np.zeros(1, KF_SCALES_DTYPE)
    rec["n_levels"], rec["th_depth"] = len(sf), np.float32(th_depth)
    rec["scale_factors"][0, :min(len(sf), 16)] = sf[:16]
    return rec


def pack_reference(slot_arrays):
    """the slot arrays (int32, a point index or -1 per keypoint) of the keyframes -> (COV_KEYFRAME_DTYPE table with HOST addresses, the
    list of arrays that keeps those addresses alive)"""
    keep = [np.ascontiguousarray(s, np.int32).reshape(-1) for s in slot_arrays]
    table = np.zeros(len(keep), COV_KEYFRAME_DTYPE)
    for k, s in enumerate(keep):
        table[k]["n_keys"], table[k]["slots"] = len(s), s.ctypes.data if len(s) else 0
    return table, keep


def _call(S, cap, new_cap, p_cap, frame_shift, point_stride, observed_offset, ref_kf_stride, n_kf, n_map_points, mode, flags, **pointers):
    call = _lib.KfCall()
    for k in _lib.KF_CALL_POINTERS:
        setattr(call, k, _lib.ptr(pointers.get(k)))
    for k, v in zip(_lib.KF_CALL_COUNTS, (S, cap, new_cap, p_cap, frame_shift, point_stride, observed_offset, ref_kf_stride, n_kf,
                                           n_map_points, mode, flags)):
        setattr(call, k, int(v))
    return call


def keyframe_insertion(scales, flags, mode=KF_MODE_KEYFRAME, *, depth, n, keys_un=None, desc=None, cam=None, assigned=None, points=None,
                       n_points=None, outlier=None, decision=None, ref_kf=None, keyframes=None, point_bad=None, point_observations=None,
                       n_points_base=None, new_cap=None, frame_shift=0, observed_offset=OBSERVED_OFFSET, depth_selected=False, out=None):
    """orbfe_keyframe_insertion on host arrays.  depth f32 (S, cap) and n i32 (S) fix S and cap; keys_un KP_DTYPE (S, cap), desc u8
    (S, cap, 32), cam UNPROJECT_CAM_DTYPE (S); assigned i32 (S, cap) or None (every slot empty) into points (S, p_cap) records of any
    dtype whose first three floats are the position, n_points i32 (S); outlier u8 (S, cap) or None; decision KF_DECISION_DTYPE (S);
    ref_kf i32 (S); keyframes a COV_KEYFRAME_DTYPE table with host addresses (pack_reference); point_bad u8 and point_observations i32
    per map point; n_points_base i32 (S) or None.  Returns a dict: headers KF_HEADER_DTYPE (S) and, with KF_CREATE, new_points
    MAP_POINT_DTYPE (S, new_cap), new_index i32 (S, new_cap), n_new i32 (S), depth_selected f32 (S, cap) when asked for, and assigned (a
    copy, as the call left it).  Arrays given in `out` are written in place: what the call does not write keeps its bytes."""
    depth = np.ascontiguousarray(depth, np.float32)
    S, cap = depth.shape
    new_cap = cap if new_cap is None else int(new_cap)
    n = np.ascontiguousarray(n, np.int32)
    c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
    keys_un, desc, cam = c(keys_un, KP_DTYPE), c(desc, np.uint8), c(cam, UNPROJECT_CAM_DTYPE)
    outlier, decision, ref_kf = c(outlier, np.uint8), c(decision, KF_DECISION_DTYPE), c(ref_kf, np.int32)
    keyframes, point_bad, point_observations = c(keyframes, COV_KEYFRAME_DTYPE), c(point_bad, np.uint8), c(point_observations, np.int32)
    n_points, n_points_base = c(n_points, np.int32), c(n_points_base, np.int32)
    out = {} if out is None else out
    if assigned is not None:
        out["assigned"] = np.array(assigned, np.int32, order="C").reshape(S, cap)
        points = np.ascontiguousarray(points)
        p_cap, point_stride = points.reshape(S, -1).shape[1], points.dtype.itemsize
        if points.dtype.fields is None:
            raise ValueError("points: an array of records (MAP_POINT_DTYPE, LAST_POINT_DTYPE, ...)")
    else:
        p_cap, point_stride, points = 1, MAP_POINT_DTYPE.itemsize, None
    out.setdefault("headers", np.zeros(S, KF_HEADER_DTYPE))
    if flags & KF_CREATE:
        out.setdefault("new_points", np.zeros((S, new_cap), MAP_POINT_DTYPE))
        out.setdefault("new_index", np.zeros((S, new_cap), np.int32))
        out.setdefault("n_new", np.zeros(S, np.int32))
        if depth_selected:
            out.setdefault("depth_selected", np.zeros((S, cap), np.float32))
    scales = np.ascontiguousarray(scales, KF_SCALES_DTYPE).reshape(1)
    call = _call(S, cap, new_cap, p_cap, frame_shift, point_stride, observed_offset, 4, 0 if keyframes is None else len(keyframes),
                 0 if point_bad is None else len(point_bad), mode, flags, keys_un=keys_un, desc=desc, depth=depth, n=n, cam=cam,
                 assigned=out.get("assigned"), points=points, n_points=n_points, outlier=outlier, decision=decision, ref_kf=ref_kf,
                 keyframes=keyframes, point_bad=point_bad, point_observations=point_observations, n_points_base=n_points_base,
                 headers=out["headers"], new_points=out.get("new_points"), new_index=out.get("new_index"), n_new=out.get("n_new"),
                 depth_selected=out.get("depth_selected"))
    _lib.check(_lib.lib().orbfe_keyframe_insertion(C.byref(call), _lib.ptr(scales)), "orbfe_keyframe_insertion")
    return out


def keyframe_insertion_device(scales, flags, mode, *, S, cap, new_cap, depth, n, headers, keys_un=None, desc=None, cam=None, assigned=None,
                              points=None, point_stride=MAP_POINT_DTYPE.itemsize, n_points=None, p_cap=1, frame_shift=0,
                              observed_offset=OBSERVED_OFFSET, outlier=None, decision=None, ref_kf=None, ref_kf_stride=4, keyframes=None,
                              n_kf=0, point_bad=None, point_observations=None, n_map_points=0, n_points_base=None, new_points=None,
                              new_index=None, n_new=None, depth_selected=None, stream=None):
    """orbfe_keyframe_insertion_batch_device: every array a torch CUDA tensor (or an int device address for ref_kf, e.g. that of the
    ref_kf field of an LM_HEADER_DTYPE array with ref_kf_stride = 32), laid out as keyframe_insertion states; scales a host
    KF_SCALES_DTYPE record.  Asynchronous on stream (a torch.cuda.Stream, or None for the NULL stream)."""
    scales = np.ascontiguousarray(scales, KF_SCALES_DTYPE).reshape(1)
    call = _call(S, cap, new_cap, p_cap, frame_shift, point_stride, observed_offset, ref_kf_stride, n_kf, n_map_points, mode, flags,
                 keys_un=keys_un, desc=desc, depth=depth, n=n, cam=cam, assigned=assigned, points=points, n_points=n_points, outlier=outlier,
                 decision=decision, keyframes=keyframes, point_bad=point_bad, point_observations=point_observations,
                 n_points_base=n_points_base, headers=headers, new_points=new_points, new_index=new_index, n_new=n_new,
                 depth_selected=depth_selected)
    call.ref_kf = C.c_void_p(ref_kf) if isinstance(ref_kf, int) else _lib.ptr(ref_kf)
    _lib.check(_lib.lib().orbfe_keyframe_insertion_batch_device(C.byref(call), _lib.ptr(scales), _lib.stream_handle(stream)),
               "orbfe_keyframe_insertion_batch_device")


# ---- the four call sites, on a batch and on one frame
def need_new_keyframe_batch(scales, **arrays):
    """Tracking::TrackLocalMap's statistics and Tracking::NeedNewKeyFrame for every frame: headers KF_HEADER_DTYPE (S)"""
    return keyframe_insertion(scales, KF_STATISTICS | KF_DECISION, KF_MODE_KEYFRAME, **arrays)["headers"]


def create_new_keyframe_batch(scales, decide=False, **arrays):
    """the points of Tracking::CreateNewKeyFrame; decide: the statistics and the decision first, points only where need == 1"""
    return keyframe_insertion(scales, KF_CREATE | (KF_STATISTICS | KF_DECISION if decide else 0), KF_MODE_KEYFRAME, **arrays)


def update_last_frame_points_batch(scales, **arrays):
    """the temporal points of Tracking::UpdateLastFrame (the caller tests :728-730)"""
    return keyframe_insertion(scales, KF_CREATE, KF_MODE_LAST_FRAME, **arrays)


def stereo_initialization_batch(scales, **arrays):
    """the points of Tracking::StereoInitialization: nothing for a frame with n <= 500"""
    return keyframe_insertion(scales, KF_CREATE, KF_MODE_STEREO_INIT, **arrays)


def _one(arrays):
    """a frame's arrays -> a batch of one"""
    lead = {"depth", "keys_un", "desc", "assigned", "points", "outlier"}
    out = {}
    for k, v in arrays.items():
        if v is None or k in ("keyframes", "point_bad", "point_observations", "new_cap", "frame_shift", "observed_offset", "depth_selected"):
            out[k] = v
        elif k in lead:
            out[k] = np.asarray(v)[None]
        else:
            out[k] = np.asarray(v).reshape(1)
    return out


def _first(res):
    return {k: v[0] for k, v in res.items()}


def need_new_keyframe(scales, **frame):
    """one frame: depth (cap), n, assigned (cap), points (p_cap), n_points, outlier, decision (a record), ref_kf and the tables"""
    return need_new_keyframe_batch(scales, **_one(frame))[0]


def create_new_keyframe(scales, decide=False, **frame):
    return _first(create_new_keyframe_batch(scales, decide, **_one(frame)))


def update_last_frame_points(scales, **frame):
    return _first(update_last_frame_points_batch(scales, **_one(frame)))


def stereo_initialization(scales, **frame):
    return _first(stereo_initialization_batch(scales, **_one(frame)))
