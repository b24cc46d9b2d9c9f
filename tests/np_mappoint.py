"""Yardstick of MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (Source/Libraries/ORB_SLAM2/src/MapPoint.cc:
229-320, :340-381), read twice.

  literal    the function as written: the live descriptors in a list, the N x N distances, `sorted(row)[int(0.5 * (N - 1))]`,
             `median < BestMedian`
  counting   what the device evaluates: per row the least value v in 0 .. 256 with |{j : d_ij <= v}| >= k + 1, the winner as the
             least (median << 16) | i

The floats are read step by step in np.float32 / np.float64 as csrc/mappoint_internal.h states them: `pos - Ow` a float difference,
cv::norm a double sum in element order and a double sqrt, `x / norm` a product with (float)(1.0 / norm), the sum sequential in list
order from 0.0f, `normal / n` a product with (float)(1.0 / n).

A point is an ordered observation list (keyframe, keypoint index) plus a position; the order stands for the iteration order of the
reference's std::map<KeyFrame*, size_t> and is part of the input.

`variant` switches ONE deviation on, so that tests/test_mappoint_cpu.py can assert that the case list tells each from the reference:
  last_wins   `<=` on a tied best median            ceil        the median index N // 2
  no_self     the self-distance left out of a row   ignore_bad  the isBad() flags not read
  eight_bits  distances kept in eight bits
"""
from __future__ import annotations

import numpy as np

UPDATE_DTYPE = np.dtype([("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("best", "<i4"), ("n_live", "<i4"),
                         ("status", "<i4"), ("desc", "u1", (32,))])
DESCRIPTOR, NORMAL_DEPTH = 1, 2
UPDATED, UNCHANGED, REFUSED = 0, 1, 2
MAX_OBS = 1024
VARIANTS = ("last_wins", "ceil", "no_self", "ignore_bad", "eight_bits")
SIZES_CPU = (1, 2, 3, 4, 5, 7, 8, 16, 31, 63, 64, 65, 66, 100)
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def distances(descs):
    """(N, 32) uint8 -> (N, N) Hamming distances"""
    d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    return _POP[d[:, None, :] ^ d[None, :, :]].sum(axis=2, dtype=np.int32)


# ---- the descriptor ----------------------------------------------------------------------------------------------------------------
def literal_descriptor(descs, bad, variant=None):
    """descs: (n, 32) uint8 in list order; bad: n flags.  Returns (best position in the list or -1, N)."""
    n = len(descs)
    if n == 0:
        return -1, 0
    live = [j for j in range(n) if variant == "ignore_bad" or not bad[j]]
    if not live:
        return -1, 0
    N = len(live)
    D = distances(np.asarray(descs)[live]).tolist()
    if variant == "eight_bits":
        D = [[x & 0xFF for x in row] for row in D]
    best_median, best_idx = 2 ** 31 - 1, 0
    for i in range(N):
        row = list(D[i])
        if variant == "no_self":
            del row[i]
        v = sorted(row)
        if variant == "ceil":
            k = N // 2
        elif variant == "no_self":
            k = int(0.5 * (len(row) - 1)) if row else 0
        else:
            k = int(0.5 * (N - 1))
        median = v[k] if v else 0
        if median < best_median or (variant == "last_wins" and median == best_median):
            best_median, best_idx = median, i
    return live[best_idx], N


def counting_descriptor(descs, bad):
    n = len(descs)
    live = [j for j in range(n) if not bad[j]]
    if n == 0 or not live:
        return -1, 0
    N = len(live)
    D = distances(np.asarray(descs)[live])
    k = (N - 1) >> 1
    best = None
    for i in range(N):
        cum = np.cumsum(np.bincount(D[i], minlength=257))
        median = int(np.argmax(cum >= k + 1))
        key = (median << 16) | i
        best = key if best is None or key < best else best
    return live[best & 0xFFFF], N


# ---- the floats --------------------------------------------------------------------------------------------------------------------
def _norm(d):
    s = np.float64(0.0)
    for k in range(3):
        s = s + np.float64(d[k]) * np.float64(d[k])
    return np.sqrt(s)


def literal_normal_depth(pos, centres, ref, ref_octave, scale_factors):
    """pos: 3 float32; centres: (n, 3) float32 in list order.  Returns (normal[3], min_distance, max_distance) as float32."""
    pos = np.asarray(pos, np.float32)
    centres = np.asarray(centres, np.float32).reshape(-1, 3)
    sf = np.asarray(scale_factors, np.float32)
    n = len(centres)
    total = [np.float32(0.0)] * 3
    with np.errstate(all="ignore"):
        for Ow in centres:
            d = [np.float32(pos[k] - Ow[k]) for k in range(3)]
            r = np.float32(np.float64(1.0) / _norm(d))
            total = [np.float32(total[k] + np.float32(d[k] * r)) for k in range(3)]
        inv_n = np.float32(np.float64(1.0) / np.float64(n))
        normal = np.array([np.float32(total[k] * inv_n) for k in range(3)], np.float32)
        PC = [np.float32(pos[k] - centres[ref][k]) for k in range(3)]
        dist = np.float32(_norm(PC))
        max_distance = np.float32(dist * sf[ref_octave])
        min_distance = np.float32(max_distance / sf[len(sf) - 1])
    return normal, min_distance, max_distance


# ---- a whole batch -----------------------------------------------------------------------------------------------------------------
def point_ok(scene, p):
    """what the device checks of a point before it reads anything else of it"""
    kfs, n_levels = scene["keyframes"], len(scene["scale_factors"])
    n = len(p["obs"])
    if n > MAX_OBS:
        return False
    if n and not (0 <= p["ref"] < n and 0 <= p["ref_octave"] < n_levels):
        return False
    return all(0 <= kf < len(kfs) and 0 <= idx < len(kfs[kf]["desc"]) for kf, idx in p["obs"])


def run(scene, flags=DESCRIPTOR | NORMAL_DEPTH, reading="literal", variant=None, prior=None):
    """The records a call leaves: the status always, the halves `flags` selects; everything else as in `prior` (zeros by default)."""
    pts, kfs = scene["points"], scene["keyframes"]
    out = np.zeros(len(pts), UPDATE_DTYPE) if prior is None else prior.copy()
    for i, p in enumerate(pts):
        ok, n = point_ok(scene, p), len(p["obs"])
        out[i]["status"] = REFUSED if not ok else UNCHANGED if n == 0 else UPDATED
        if flags & DESCRIPTOR:
            out[i]["best"], out[i]["n_live"], out[i]["desc"] = -1, 0, 0
        if flags & NORMAL_DEPTH:
            out[i]["normal"], out[i]["min_distance"], out[i]["max_distance"] = 0, 0, 0
        if not ok or n == 0:
            continue
        if flags & DESCRIPTOR:
            descs = np.stack([kfs[kf]["desc"][idx] for kf, idx in p["obs"]])
            bad = [kfs[kf]["bad"] for kf, _ in p["obs"]]
            best, N = literal_descriptor(descs, bad, variant) if reading == "literal" else counting_descriptor(descs, bad)
            out[i]["best"], out[i]["n_live"] = best, N
            if best >= 0:
                out[i]["desc"] = descs[best]
        if flags & NORMAL_DEPTH:
            centres = np.stack([kfs[kf]["Ow"] for kf, _ in p["obs"]])
            nrm, mn, mx = literal_normal_depth(p["pos"], centres, p["ref"], p["ref_octave"], scene["scale_factors"])
            out[i]["normal"], out[i]["min_distance"], out[i]["max_distance"] = nrm, mn, mx
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def scale_factors(n_levels=8, scale=1.2):
    sf = [np.float32(1.0)]
    for _ in range(1, n_levels):
        sf.append(np.float32(sf[-1] * np.float32(scale)))
    return np.array(sf, np.float32)


def make_scene(seed, sizes, bad_frac=0.15, n_levels=8, max_flips=39):
    """One point per entry of `sizes` (its number of observations).  A point's descriptors are a base descriptor with 0 .. max_flips
    random bits flipped per observation -- such families have tied medians, uniformly random descriptors do not --, about bad_frac of
    the keyframes are bad, and a point's observations name distinct keyframes in a random order (the std::map's pointer order)."""
    rng = np.random.default_rng(seed)
    P = len(sizes)
    n_kf = max(max(sizes, default=1), 8) + 16
    rows = P + 3
    kfs = []
    for _ in range(n_kf):
        kfs.append(dict(desc=rng.integers(0, 256, (rows, 32), dtype=np.uint8), bad=bool(rng.random() < bad_frac),
                        Ow=rng.uniform(-5, 5, 3).astype(np.float32), perm=rng.permutation(rows)))
    pts = []
    for i, n in enumerate(sizes):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        order = rng.permutation(n_kf)[:n]
        obs = []
        for kf in order:
            idx = int(kfs[kf]["perm"][i])
            bits = np.unpackbits(base)
            flips = rng.permutation(256)[:rng.integers(0, max_flips + 1)]
            bits[flips] ^= 1
            kfs[kf]["desc"][idx] = np.packbits(bits)
            obs.append((int(kf), idx))
        pos = (rng.uniform(-20, 20, 3) + np.array([0, 0, 40.0])).astype(np.float32)
        pts.append(dict(obs=obs, pos=pos, ref=int(rng.integers(0, n)) if n else 0, ref_octave=int(rng.integers(0, n_levels))))
    for kf in kfs:
        del kf["perm"]
    return dict(keyframes=kfs, points=pts, scale_factors=scale_factors(n_levels))


def nine_bit_scene():
    """{a ^ 1, a, ~a, ~a}: rows {0,1,255,255} {1,0,256,256} {255,256,0,0} {255,256,0,0}, medians 1 1 0 0 -> index 2.  With the 256 kept
    in eight bits row 1 is {1,0,0,0} and wins with median 0."""
    a = np.arange(32, dtype=np.uint8) * 7 + 3
    a1 = a.copy()
    a1[0] ^= 1
    descs = [a1, a, ~a, ~a]
    kfs = [dict(desc=np.stack([d]), bad=False, Ow=np.array([k, 0.5 * k, -1.0], np.float32)) for k, d in enumerate(descs)]
    pts = [dict(obs=[(k, 0) for k in range(4)], pos=np.array([1.0, 2.0, 30.0], np.float32), ref=1, ref_octave=2)]
    return dict(keyframes=kfs, points=pts, scale_factors=scale_factors())


def cpu_cases():
    """84 one-point scenes: six seeds of every size of SIZES_CPU"""
    return [make_scene(1000 * n + s, [n]) for n in SIZES_CPU for s in range(6)]
