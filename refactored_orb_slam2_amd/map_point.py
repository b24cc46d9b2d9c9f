"""MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth over the C ABI of liborbfe.so (L/src/MapPoint.cc:229-320,
:340-381, L/ = Source/Libraries/ORB_SLAM2/): the descriptor with the least median Hamming distance to the other observations, the mean
viewing direction and the scale-invariance range, for a batch of map points at once.

A point is an ORDERED list of observations (keyframe, keypoint index) -- the iteration order of the reference's std::map, which the
caller states -- plus a position.  refresh_map_points takes Python structures, refresh_map_points_batch the packed records on host
arrays, refresh_map_points_device the same records on device tensors.  All three run mappoint_kernels.hip; there is no CPU path.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import (MP_DESCRIPTOR, MP_KEYFRAME_DTYPE, MP_NORMAL_DEPTH, MP_OBS_DTYPE, MP_POINT_DTYPE, MP_REFUSED, MP_UNCHANGED,
                   MP_UPDATE_DTYPE, MP_UPDATED)

__all__ = ["MP_KEYFRAME_DTYPE", "MP_OBS_DTYPE", "MP_POINT_DTYPE", "MP_UPDATE_DTYPE", "MP_DESCRIPTOR", "MP_NORMAL_DEPTH", "MP_UPDATED",
           "MP_UNCHANGED", "MP_REFUSED", "pack_map_points", "refresh_map_points", "refresh_map_points_batch",
           "refresh_map_points_device"]


def pack_map_points(keyframes, points):
    """Python structures -> the packed records.  keyframes: a list of dicts with desc ((n, 32) uint8 = mDescriptors), bad (isBad()) and
    Ow (GetCameraCenter()); points: a list of dicts with obs (a list of (keyframe index, keypoint index) in map order; empty for a bad
    point), pos, ref (position of mpRefKF in obs) and ref_octave.  Returns (table, obs, recs, positions, keep): MP_KEYFRAME_DTYPE with
    HOST addresses, MP_OBS_DTYPE, MP_POINT_DTYPE, (P, 3) float32, and the arrays the addresses point into."""
    table = np.zeros(len(keyframes), MP_KEYFRAME_DTYPE)
    keep = []
    for k, kf in enumerate(keyframes):
        d = np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32)
        keep.append(d)
        table[k]["desc"], table[k]["n_keys"] = (d.ctypes.data if len(d) else 0), len(d)
        table[k]["bad"], table[k]["Ow"] = int(bool(kf["bad"])), np.asarray(kf["Ow"], np.float32).reshape(3)
    n_total = sum(len(p["obs"]) for p in points)
    obs, recs = np.zeros(n_total, MP_OBS_DTYPE), np.zeros(len(points), MP_POINT_DTYPE)
    positions = np.zeros((len(points), 3), np.float32)
    off = 0
    for i, p in enumerate(points):
        n = len(p["obs"])
        if n:
            o = np.asarray(p["obs"], np.int32).reshape(n, 2)
            obs["kf"][off:off + n], obs["idx"][off:off + n] = o[:, 0], o[:, 1]
        recs[i] = (off, n, p.get("ref", 0), p.get("ref_octave", 0))
        positions[i] = np.asarray(p["pos"], np.float32).reshape(3)
        off += n
    return table, obs, recs, positions, keep


def refresh_map_points_batch(table, obs, recs, positions, scale_factors, flags=MP_DESCRIPTOR | MP_NORMAL_DEPTH, updates=None):
    """orbfe_refresh_map_points on host arrays: table MP_KEYFRAME_DTYPE (desc = HOST addresses), obs MP_OBS_DTYPE, recs MP_POINT_DTYPE,
    positions (P, 3) float32, scale_factors = mvScaleFactors.  Returns MP_UPDATE_DTYPE (P): the status and the halves `flags` selects
    are written (into `updates` when given, whose other bytes stay)."""
    table = np.ascontiguousarray(table, MP_KEYFRAME_DTYPE)
    obs = np.ascontiguousarray(obs, MP_OBS_DTYPE)
    recs = np.ascontiguousarray(recs, MP_POINT_DTYPE)
    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    if len(positions) != len(recs):
        raise ValueError("one position per point")
    out = np.zeros(len(recs), MP_UPDATE_DTYPE) if updates is None else updates
    if out.dtype != MP_UPDATE_DTYPE or len(out) != len(recs) or not out.flags.c_contiguous:
        raise ValueError("updates: a contiguous MP_UPDATE_DTYPE array with one record per point")
    _lib.check(_lib.lib().orbfe_refresh_map_points(_lib.ptr(table), len(table), _lib.ptr(obs), len(obs), _lib.ptr(recs), _lib.ptr(positions),
                                                   len(recs), _lib.ptr(sf), len(sf), int(flags), _lib.ptr(out)), "orbfe_refresh_map_points")
    return out


def refresh_map_points(keyframes, points, scale_factors, flags=MP_DESCRIPTOR | MP_NORMAL_DEPTH):
    """Both functions for a list of points (see pack_map_points).  Returns MP_UPDATE_DTYPE (P): best = position in the point's own
    list of the chosen descriptor (-1: none), desc, n_live, normal, min_distance, max_distance, status."""
    table, obs, recs, positions, keep = pack_map_points(keyframes, points)
    out = refresh_map_points_batch(table, obs, recs, positions, scale_factors, flags)
    del keep
    return out


def refresh_map_points_device(table, obs, recs, positions, point_stride, scale_factors, flags, updates, stream=None):
    """orbfe_refresh_map_points_batch_device on torch CUDA tensors: table (n_kf, 32) u8 = MP_KEYFRAME_DTYPE with DEVICE addresses,
    obs (n_obs_total, 8) u8, recs (P, 16) u8, positions: P records point_stride bytes apart with the position first, updates (P, 64) u8
    = MP_UPDATE_DTYPE.  scale_factors stays on the host.  Asynchronous on stream (a torch.cuda.Stream, or None for the NULL stream)."""
    sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    _lib.check(_lib.lib().orbfe_refresh_map_points_batch_device(int(recs.shape[0]), _lib.ptr(table), int(table.shape[0]), _lib.ptr(obs),
                                                                int(obs.shape[0]), _lib.ptr(recs), _lib.ptr(positions), int(point_stride),
                                                                _lib.ptr(sf), len(sf), int(flags), _lib.ptr(updates),
                                                                _lib.stream_handle(stream)), "orbfe_refresh_map_points_batch_device")
