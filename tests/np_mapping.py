"""A numpy reading of the triangulation half of LocalMapping::CreateNewMapPoints (L/src/LocalMapping.cc:261-402, L/ =
Source/Libraries/ORB_SLAM2/), KeyFrame::UnprojectStereo (L/src/KeyFrame.cc:573-586) and MapPoint::UpdateNormalAndDepth
(L/src/MapPoint.cc:340-381): the yardstick of tests/test_mapping_cpu.py and tests/test_mapping_gpu.py.  Written from the reference's
source, not from csrc/mapping_internal.h, and structured differently on purpose: every step is a numpy column over all pairs, the
gates are masks applied in the reference's order, and the decomposition is numpy.linalg.svd.

Two modes:
  R64  every operation in float64 on the float32 inputs, SVD by LAPACK's double driver.  The truth.
  R32  elementwise arithmetic in numpy.float32 in the reference's order (Mat::dot and cv::norm accumulate in double and their
       results are rounded once, comparisons against the double literals 5.991 / 7.8 / 0.9998 are made in double), SVD by
       numpy.linalg.svd on the float32 matrix = LAPACK's single-precision driver, which is what an OpenCV built with LAPACK calls.
       It stands in for the reference's float result.

Each pair also gets a margin verdict (R64): it is a PARITY pair when every parallax comparison that steers it is at least 64 float
ulps wide and every gate it reaches is at least 1e-3 (relative) away from its threshold; only those pairs can be compared code for
code between two implementations whose atan2 / cos / SVD differ in the last bits."""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
MAX_LEVELS = 16
(OK, NO_MATCH, W_ZERO, LOW_PARALLAX, BEHIND1, BEHIND2, REPROJ1, REPROJ2, DIST_ZERO, SCALE) = range(10)
CODE_NAMES = ("ok", "no_match", "w_zero", "low_parallax", "behind1", "behind2", "reproj1", "reproj2", "dist_zero", "scale")
REACHABLE = (OK, NO_MATCH, LOW_PARALLAX, BEHIND1, BEHIND2, REPROJ1, REPROJ2, SCALE)   # w == 0 and dist == 0 need exact zeros
PATH_NONE, PATH_LINEAR, PATH_UNPROJECT1, PATH_UNPROJECT2 = range(4)
PARALLAX_ULPS, GATE_MARGIN = 64, 1e-3
NON_PARITY_CAP = 0.02   # of a case's pairs

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                       ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4"), ("mb", "<f4"), ("mbf", "<f4"), ("n_levels", "<i4"),
                       ("scale_factors", "<f4", (16,)), ("level_sigma2", "<f4", (16,))])
POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"),
                        ("idx2", "<i4"), ("code", "<i4"), ("path", "<i4")])

KITTI = dict(fx=718.856, fy=718.856, cx=607.19, cy=185.2, mb=0.537)


def make_view(R, t, n_levels=8, scale=1.2, cam=KITTI):
    """One orbfe_tri_view record from a double pose (Rcw, tcw): everything the KeyFrame would hold, rounded to float as it does."""
    v = np.zeros(1, VIEW_DTYPE)
    R32, t32 = np.asarray(R, F64).astype(F32), np.asarray(t, F64).astype(F32)
    v["Rcw"][0], v["tcw"][0] = R32.reshape(9), t32
    v["Ow"][0] = (-(R32.astype(F64).T @ t32.astype(F64))).astype(F32)     # Ow = -Rwc * tcw (KeyFrame::SetPose)
    fx, fy = F32(cam["fx"]), F32(cam["fy"])
    v["fx"], v["fy"], v["cx"], v["cy"] = fx, fy, cam["cx"], cam["cy"]
    v["invfx"], v["invfy"] = F32(1.0) / fx, F32(1.0) / fy
    v["mb"] = cam["mb"]
    v["mbf"] = F32(cam["mb"]) * fx
    v["n_levels"] = n_levels
    sf = np.ones(MAX_LEVELS, F32)
    for i in range(1, MAX_LEVELS):
        sf[i] = sf[i - 1] * F32(scale)                                   # ORBextractor: mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor
    v["scale_factors"][0] = sf
    v["level_sigma2"][0] = sf * sf
    return v


def _ulps_apart(a, b, n):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.abs(a - b) >= n * np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F32)).astype(F64)


def _dotd(a, b):
    """Mat::dot / the sum under cv::norm: double accumulation in element order; a, b are lists of three columns"""
    s = a[0].astype(F64) * b[0].astype(F64)
    s = s + a[1].astype(F64) * b[1].astype(F64)
    return s + a[2].astype(F64) * b[2].astype(F64)


def triangulate(view1, view2, keys1, ur1, depth1, keys2, ur2, depth2, matchA, mode="R64"):
    """All pairs (i, matchA[i]) of one (pKF1, pKF2).  Returns a dict of columns over the nA features of pKF1: code, path, idx2, pos,
    normal, min_distance, max_distance, parity (bool; meaningful in R64)."""
    assert mode in ("R64", "R32")
    T = F64 if mode == "R64" else F32
    v1, v2 = np.asarray(view1).reshape(-1)[0], np.asarray(view2).reshape(-1)[0]
    nA, nB = len(keys1), len(keys2)
    matchA = np.asarray(matchA, np.int64)
    res = dict(code=np.full(nA, NO_MATCH, np.int32), path=np.zeros(nA, np.int32), idx2=np.full(nA, -1, np.int32),
               pos=np.zeros((nA, 3), T), normal=np.zeros((nA, 3), T), min_distance=np.zeros(nA, T), max_distance=np.zeros(nA, T),
               parity=np.ones(nA, bool))
    L1, L2 = int(v1["n_levels"]), int(v2["n_levels"])
    m = (matchA >= 0) & (matchA < nB)
    j = np.where(m, matchA, 0)
    o1, o2 = keys1["octave"].astype(np.int64), (keys2["octave"].astype(np.int64)[j] if nB else np.zeros(nA, np.int64))
    m &= (o1 >= 0) & (o1 < L1) & (o2 >= 0) & (o2 < L2)
    rows = np.nonzero(m)[0]
    if len(rows) == 0:
        return res
    j, o1, o2 = j[rows], o1[rows], o2[rows]
    n = len(rows)
    c = lambda x: np.asarray(x, F32).astype(T)                            # a float of the ABI in the working type
    x1, y1, x2, y2 = c(keys1["x"][rows]), c(keys1["y"][rows]), c(keys2["x"][j]), c(keys2["y"][j])
    u1r = c(ur1[rows]) if ur1 is not None else np.full(n, -1, T)
    u2r = c(ur2[j]) if ur2 is not None else np.full(n, -1, T)
    st1, st2 = u1r >= 0, u2r >= 0
    z1o = c(depth1[rows]) if depth1 is not None else np.full(n, -1, T)
    z2o = c(depth2[j]) if depth2 is not None else np.full(n, -1, T)
    R1, R2 = c(v1["Rcw"]).reshape(3, 3), c(v2["Rcw"]).reshape(3, 3)
    t1, t2, Ow1, Ow2 = c(v1["tcw"]), c(v2["tcw"]), c(v1["Ow"]), c(v2["Ow"])
    K1 = [c(v1[k]) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy")]
    K2 = [c(v2[k]) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy")]
    one = np.ones(n, T)
    with np.errstate(all="ignore"):
        # :274-282
        xn1 = [(x1 - K1[2]) * K1[4], (y1 - K1[3]) * K1[5], one]
        xn2 = [(x2 - K2[2]) * K2[4], (y2 - K2[3]) * K2[5], one]
        ray1 = [R1[0, r] * xn1[0] + R1[1, r] * xn1[1] + R1[2, r] * xn1[2] for r in range(3)]      # Rwc = Rcw.t()
        ray2 = [R2[0, r] * xn2[0] + R2[1, r] * xn2[1] + R2[2, r] * xn2[2] for r in range(3)]
        cpr = (_dotd(ray1, ray2) / (np.sqrt(_dotd(ray1, ray1)) * np.sqrt(_dotd(ray2, ray2)))).astype(T)
        # :284-294
        cps1 = cpr + T(1)
        cps2 = cps1.copy()
        mb1, mb2 = c(v1["mb"]), c(v2["mb"])
        s1 = np.cos(T(2) * np.arctan2(np.full(n, mb1 / T(2), T), z1o))
        s2 = np.cos(T(2) * np.arctan2(np.full(n, mb2 / T(2), T), z2o))
        cps1 = np.where(st1, s1, cps1).astype(T)
        cps2 = np.where(~st1 & st2, s2, cps2).astype(T)
        cps = np.minimum(cps1, cps2)
        any_st = st1 | st2
        linear = (cpr < cps) & (cpr > 0) & (any_st | (cpr.astype(F64) < 0.9998))
        unp1 = ~linear & st1 & (cps1 < cps2)
        unp2 = ~linear & ~unp1 & st2 & (cps2 < cps1)
        path = np.where(linear, PATH_LINEAR, np.where(unp1, PATH_UNPROJECT1, np.where(unp2, PATH_UNPROJECT2, PATH_NONE)))
        par = _ulps_apart(cpr, cps, PARALLAX_ULPS) & (np.abs(cpr.astype(F64)) >= PARALLAX_ULPS * 2.0 ** -24)   # against 0: ulps of the unit rays
        par &= any_st | _ulps_apart(cpr, np.full(n, 0.9998), PARALLAX_ULPS)
        par &= ~any_st | _ulps_apart(cps1, cps2, PARALLAX_ULPS)
        # :300-315
        Tc1, Tc2 = np.concatenate([R1, t1[:, None]], 1), np.concatenate([R2, t2[:, None]], 1)
        A = np.empty((n, 4, 4), T)
        for col in range(4):
            A[:, 0, col] = xn1[0] * Tc1[2, col] - Tc1[0, col]
            A[:, 1, col] = xn1[1] * Tc1[2, col] - Tc1[1, col]
            A[:, 2, col] = xn2[0] * Tc2[2, col] - Tc2[0, col]
            A[:, 3, col] = xn2[1] * Tc2[2, col] - Tc2[1, col]
        A = np.where(np.isfinite(A), A, 0)
        vt = np.linalg.svd(A)[2]
        assert vt.dtype == T
        h = vt[:, 3, :]
        w_zero = linear & (h[:, 3] == 0)
        xl = [h[:, k] / h[:, 3] for k in range(3)]
        # KeyFrame::UnprojectStereo
        def unproject(R, Ow, K, x, y, z):
            xc, yc = (x - K[2]) * z * K[4], (y - K[3]) * z * K[5]
            return [R[0, r] * xc + R[1, r] * yc + R[2, r] * z + Ow[r] for r in range(3)]
        xu1, xu2 = unproject(R1, Ow1, K1, x1, y1, z1o), unproject(R2, Ow2, K2, x2, y2, z2o)
        X = [np.where(linear, xl[k], np.where(unp1, xu1[k], xu2[k])).astype(T) for k in range(3)]
        code = np.full(n, -1, np.int32)
        def reject(mask, value):
            nonlocal code
            code = np.where((code < 0) & mask, value, code)
        live = lambda: code < 0
        reject(w_zero, W_ZERO)
        reject(path == PATH_NONE, LOW_PARALLAX)
        # :327-333
        cam = lambda R, t, r: (_dotd([np.full(n, R[r, 0], T), np.full(n, R[r, 1], T), np.full(n, R[r, 2], T)], X) + F64(t[r])).astype(T)
        n1v, n2v = [X[k] - Ow1[k] for k in range(3)], [X[k] - Ow2[k] for k in range(3)]
        d1, d2 = np.sqrt(_dotd(n1v, n1v)), np.sqrt(_dotd(n2v, n2v))      # double, as cv::norm returns them
        z1 = cam(R1, t1, 2)
        par &= ~live() | (np.abs(z1.astype(F64)) >= GATE_MARGIN * d1)
        reject(z1 <= 0, BEHIND1)
        z2 = cam(R2, t2, 2)
        par &= ~live() | (np.abs(z2.astype(F64)) >= GATE_MARGIN * d2)
        reject(z2 <= 0, BEHIND2)
        # :336-382
        mbf1 = c(v1["mbf"])
        def reproj(R, t, K, z, x, y, ur, st, sig):
            xc, yc = cam(R, t, 0), cam(R, t, 1)
            invz = (1.0 / z.astype(F64)).astype(T)
            u = K[0] * xc * invz + K[2]
            v = K[1] * yc * invz + K[3]
            u_r = u - mbf1 * invz
            ex, ey, er = u - x, v - y, u_r - ur
            e2 = np.where(st, ex * ex + ey * ey + er * er, ex * ex + ey * ey).astype(T).astype(F64)
            thr = np.where(st, 7.8, 5.991) * sig.astype(F64)
            return e2 > thr, np.abs(e2 - thr) >= GATE_MARGIN * thr
        sig1, sig2 = c(v1["level_sigma2"])[o1], c(v2["level_sigma2"])[o2]
        bad, wide = reproj(R1, t1, K1, z1, x1, y1, u1r, st1, sig1)
        par &= ~live() | wide
        reject(bad, REPROJ1)
        bad, wide = reproj(R2, t2, K2, z2, x2, y2, u2r, st2, sig2)
        par &= ~live() | wide
        reject(bad, REPROJ2)
        # :385-402
        dist1, dist2 = d1.astype(T), d2.astype(T)
        reject((dist1 == 0) | (dist2 == 0), DIST_ZERO)
        sfa, sfb = c(v1["scale_factors"]), c(v2["scale_factors"])
        rf = T(1.5) * sfa[1]
        rd, ro = dist2 / dist1, sfa[o1] / sfb[o2]
        par &= ~live() | ((np.abs(rd * rf - ro) >= GATE_MARGIN * ro) & (np.abs(rd - ro * rf) >= GATE_MARGIN * ro * rf))
        reject((rd * rf < ro) | (rd > ro * rf), SCALE)
        ok = live()
        code = np.where(ok, OK, code)
        # MapPoint::UpdateNormalAndDepth, observations {pKF1, pKF2}, pRefKF = pKF1
        nrm = [((n1v[k] / d1.astype(T) + n2v[k] / d2.astype(T)) / T(2)).astype(T) for k in range(3)]
        maxd = dist1 * sfa[o1]
        mind = maxd / sfa[L1 - 1]
    res["code"][rows], res["path"][rows], res["idx2"][rows], res["parity"][rows] = code, path, matchA[rows], par
    for k in range(3):
        res["pos"][rows, k] = np.where(ok, X[k], 0)
        res["normal"][rows, k] = np.where(ok, nrm[k], 0)
    res["max_distance"][rows], res["min_distance"][rows] = np.where(ok, maxd, 0), np.where(ok, mind, 0)
    return res


def baseline_too_short(view1, view2, monocular, median_depth):
    """:221-235, float as the reference: True = the neighbour is skipped"""
    a, b = np.asarray(view1).reshape(-1)[0], np.asarray(view2).reshape(-1)[0]
    d = (b["Ow"] - a["Ow"]).astype(F32)
    baseline = F32(np.sqrt(np.sum(d.astype(F64) ** 2)))
    if not monocular:
        return bool(baseline < b["mb"])
    return bool(F64(baseline / F32(median_depth)) < 0.01)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def yaw(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F64)


CASES = {
    "mixed": dict(seed=11, base=0.6, stereo=0.6),
    "all_mono": dict(seed=12, base=0.6, stereo=0.0),
    "short_baseline": dict(seed=13, base=0.05, stereo=0.6),
    "all_stereo": dict(seed=14, base=0.6, stereo=1.0),
    "twelve_levels": dict(seed=15, base=0.6, stereo=0.6, n_levels=12),
    # two more than the recipe needs for its statistics, for the gates it does not reach: a long stride makes near points fail the
    # scale-consistency gate and sends most pairs down the linear path; outliers that cross the epipole put the linear solution
    # between the two cameras (z1 > 0, z2 <= 0)
    "wide_baseline": dict(seed=18, base=2.9, stereo=0.3),
    "around_epipole": dict(seed=20, base=0.6, stereo=1.0, xr=1.0, yr=0.5, outliers=0.3, around_epipole=True),
}


def make_scene(seed, n=1500, base=0.6, stereo=0.6, n_levels=8, noise=True, outliers=0.08, unmatched=0.1, xr=15.0, yr=3.0, zr=(3.0, 60.0),
               around_epipole=False):
    """Two keyframes of a KITTI camera looking at n points (x +-15, y +-3, z 3..60 in the first camera), the second translated by
    (0.15, 0.02, base) with 0.03 rad of yaw; pixel noise of one pixel x level scale, gross outliers of 8 px x scale in u of the
    second view, octave from depth (+-1 in the second view), stereo observations with depth noise z^2 / mbf.  matchA is a
    permutation with `unmatched` of its entries -1."""
    rng = np.random.default_rng(seed)
    R1, t1 = yaw(0.1), np.array([1.0, -0.5, 2.0])
    Rr, tr = yaw(0.03), -yaw(0.03) @ np.array([0.15, 0.02, base])         # camera 2 sits at (0.15, 0.02, base) in camera 1
    R2, t2 = Rr @ R1, Rr @ t1 + tr
    v1, v2 = make_view(R1, t1, n_levels), make_view(R2, t2, n_levels)
    Pc1 = np.stack([rng.uniform(-xr, xr, n), rng.uniform(-yr, yr, n), rng.uniform(zr[0], zr[1], n)], 1)
    if around_epipole:                                                    # centred on the line through both camera centres
        Pc1[:, 0] += Pc1[:, 2] * 0.15 / base
        Pc1[:, 1] += Pc1[:, 2] * 0.02 / base
    Pw = (Pc1 - t1) @ R1                                                  # R1^T (Pc - t)
    Pc2 = Pw @ R2.T + t2
    sf = v1["scale_factors"][0].astype(F64)
    fx, fy, cx, cy, mb = (KITTI[k] for k in ("fx", "fy", "cx", "cy", "mb"))
    mbf = mb * fx
    oct1 = np.clip(np.round(np.log(20.0 / Pc1[:, 2]) / np.log(1.2)), 0, n_levels - 1).astype(np.int32)
    oct2 = np.clip(oct1 + rng.integers(-1, 2, n), 0, n_levels - 1).astype(np.int32)
    is_st1, is_st2 = rng.random(n) < stereo, rng.random(n) < stereo
    out = rng.random(n) < (outliers if noise else 0.0)

    def observe(Pc, octv, is_st, gross):
        s = sf[octv] if noise else 0.0
        u = fx * Pc[:, 0] / Pc[:, 2] + cx + rng.normal(0, 1, n) * s
        v = fy * Pc[:, 1] / Pc[:, 2] + cy + rng.normal(0, 1, n) * s
        u = u + np.where(gross, rng.choice([-8.0, 8.0], n) * sf[octv], 0.0)
        z = Pc[:, 2] + (rng.normal(0, 1, n) * Pc[:, 2] ** 2 / mbf if noise else 0.0)
        z = np.where(z > 0.5, z, 0.5)
        keys = np.zeros(n, KP_DTYPE)
        keys["x"], keys["y"], keys["octave"] = u, v, octv
        keys["size"], keys["angle"], keys["class_id"] = 31 * sf[octv], rng.uniform(0, 360, n), -1
        depth = np.where(is_st, z, -1.0).astype(F32)
        ur = np.where(is_st, u - mbf / z, -1.0).astype(F32)
        ur = np.where(is_st & (ur < 0), F32(0), ur)
        return keys, ur, depth

    k1, ur1, z1 = observe(Pc1, oct1, is_st1, np.zeros(n, bool))
    k2, ur2, z2 = observe(Pc2, oct2, is_st2, out)
    perm = rng.permutation(n)                                              # pKF2 stores point i at row perm[i]
    inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
    k2, ur2, z2 = k2[inv], ur2[inv], z2[inv]
    matchA = np.where(rng.random(n) < unmatched, -1, perm).astype(np.int32)
    return dict(view1=v1, view2=v2, keys1=k1, ur1=ur1, depth1=z1, keys2=k2, ur2=ur2, depth2=z2, matchA=matchA, Pw=Pw, perm=perm,
                mono=stereo == 0.0)


def case_scene(name, n=1500):
    return make_scene(n=n, **CASES[name])


def run(scene, mode):
    s = scene
    mono = s.get("mono", False)
    return triangulate(s["view1"], s["view2"], s["keys1"], None if mono else s["ur1"], None if mono else s["depth1"], s["keys2"],
                       None if mono else s["ur2"], None if mono else s["depth2"], s["matchA"], mode)


def rel_error(pos, ref):
    """error of each row of pos against ref relative to |ref|_inf (both (n, 3))"""
    ref = np.asarray(ref, F64)
    return np.abs(np.asarray(pos, F64) - ref).max(1) / np.abs(ref).max(1)


def pack_points(r):
    """the columns of triangulate() as orbfe_new_point records (R32: the bytes the library is compared with)"""
    p = np.zeros(len(r["code"]), POINT_DTYPE)
    p["pos"], p["normal"] = r["pos"], r["normal"]
    p["min_distance"], p["max_distance"] = r["min_distance"], r["max_distance"]
    p["idx2"], p["code"], p["path"] = r["idx2"], r["code"], r["path"]
    p["path"] = np.where(p["code"] == NO_MATCH, 0, p["path"])
    return p


# ---- the neighbour loop (:215-422) ---------------------------------------------------------------------------------------------------
EPIPOLAR_DTYPE = np.dtype([("F12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4"), ("scale_factors", "<f4", (16,)),
                           ("level_sigma2", "<f4", (16,))])


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], F64)


def epipolar(view1, view2):
    """LocalMapping::ComputeF12 (:556-575) and the epipole of SearchForTriangulation (ORBmatcher.cc:622-630), which stay the caller's:
    computed in double from the two float poses, one orbfe_epipolar record"""
    a, b = np.asarray(view1).reshape(-1)[0], np.asarray(view2).reshape(-1)[0]
    R1, R2 = a["Rcw"].astype(F64).reshape(3, 3), b["Rcw"].astype(F64).reshape(3, 3)
    t1, t2 = a["tcw"].astype(F64), b["tcw"].astype(F64)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    Kf = lambda v: np.array([[v["fx"], 0, v["cx"]], [0, v["fy"], v["cy"]], [0, 0, 1]], F64)
    F12 = np.linalg.inv(Kf(a)).T @ _skew(t12) @ R12 @ np.linalg.inv(Kf(b))
    C2 = R2 @ a["Ow"].astype(F64) + t2
    ep = np.zeros(1, EPIPOLAR_DTYPE)
    ep["F12"][0] = F12.reshape(9)
    ep["ex"], ep["ey"] = b["fx"] * C2[0] / C2[2] + b["cx"], b["fy"] * C2[1] / C2[2] + b["cy"]
    ep["scale_factors"][0], ep["level_sigma2"][0] = b["scale_factors"], b["level_sigma2"]
    return ep


def make_chain_scene(seed=41, n=300, monocular=False, n_levels=8, rel=None):
    """pKF1 and three neighbours looking at n points; every keyframe sees every point, in its own row order, with a descriptor that
    is the point's with three flipped bits (never in byte 0, which picks one of 40 vocabulary buckets).  Neighbour 2 stands too close:
    stereo, its baseline (0.22 m) is below mb; monocular, its median depth makes baseline / depth 0.002."""
    rng = np.random.default_rng(seed)
    R1, t1 = yaw(0.1), np.array([1.0, -0.5, 2.0])
    if rel is None:                                                       # (camera centre in pKF1's frame, yaw)
        rel = [((0.15, 0.02, 0.6), 0.03), ((-0.3, 0.01, 1.2), -0.02), ((0.1, 0.0, 0.2), 0.01)]
    fx, fy, cx, cy, mb = (KITTI[k] for k in ("fx", "fy", "cx", "cy", "mb"))
    mbf = mb * fx
    Pc1 = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(3, 60, n)], 1)
    Pw = (Pc1 - t1) @ R1
    pdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sf = make_view(R1, t1, n_levels)["scale_factors"][0].astype(F64)

    def keyframe(R, t, has_fraction):
        Pc = Pw @ R.T + t
        octv = np.clip(np.round(np.log(20.0 / Pc[:, 2]) / np.log(1.2)) + rng.integers(-1, 2, n), 0, n_levels - 1).astype(np.int32)
        order = rng.permutation(n)                                         # row r holds point order[r]
        Pc, octv = Pc[order], octv[order]
        keys = np.zeros(n, KP_DTYPE)
        keys["x"] = fx * Pc[:, 0] / Pc[:, 2] + cx + rng.normal(0, 0.5, n) * sf[octv]
        keys["y"] = fy * Pc[:, 1] / Pc[:, 2] + cy + rng.normal(0, 0.5, n) * sf[octv]
        keys["octave"], keys["size"], keys["class_id"] = octv, 31 * sf[octv], -1
        keys["angle"] = (30.0 + rng.normal(0, 2, n)) % 360                 # one rotation for all: the histogram keeps them
        is_st = (rng.random(n) < 0.6) & (not monocular)
        z = np.maximum(Pc[:, 2] + rng.normal(0, 1, n) * Pc[:, 2] ** 2 / mbf, 0.5)
        ur = np.where(is_st, np.maximum(keys["x"] - mbf / z, 0), -1.0).astype(F32)
        depth = np.where(is_st, z, -1.0).astype(F32)
        desc = pdesc[order].copy()
        for _ in range(3):                                                 # three flips per row (a bit hit twice flips back)
            b = rng.integers(8, 256, n)
            desc[np.arange(n), b // 8] ^= (1 << (b % 8)).astype(np.uint8)
        groups = {}
        for r in range(n):
            groups.setdefault(int(desc[r, 0]) % 40, []).append(r)
        has = (rng.random(n) < has_fraction).astype(np.uint8)
        return dict(keys=keys, desc=desc, u_right=None if monocular else ur, depth=None if monocular else depth, has_mp=has,
                    groups=groups, view=make_view(R, t, n_levels), order=order)

    A = keyframe(R1, t1, 0.2)
    nbs = []
    for (c, a) in rel:
        Rr = yaw(a)
        nb = keyframe(Rr @ R1, Rr @ t1 - Rr @ np.array(c), 0.1)
        nb["epipolar"] = epipolar(A["view"], nb["view"])
        nb["median_depth"] = 100.0 if c[2] < 0.5 else 30.0
        nbs.append(nb)
    return dict(A=A, neighbors=nbs, monocular=monocular)


def replay_chain(scene, search, device_points=None, only_stereo=False, check_orientation=True):
    """The loop of :215-422 on the yardsticks: per neighbour the gate, `search` (tests/oracle_lib.search_for_triangulation), the R32
    reading, the mask update.  At a pair that is not a parity pair (R64 margins) the replay adopts device_points' code, so that one
    borderline decision does not change every later neighbour; the count of such pairs is returned for the caller's cap.
    Returns (points [K][nA] POINT_DTYPE, n_matches, n_new, has_mp, adopted, searched) -- searched[k] = the matchA of neighbour k."""
    A, nbs, mono = scene["A"], scene["neighbors"], scene["monocular"]
    nA, K = len(A["keys"]), len(nbs)
    has = A["has_mp"].copy()
    pts = np.zeros((K, nA), POINT_DTYPE)
    pts["idx2"], pts["code"] = -1, NO_MATCH
    n_matches, n_new, adopted, searched = np.zeros(K, np.int32), np.zeros(K, np.int32), 0, []
    for k, nb in enumerate(nbs):
        if baseline_too_short(A["view"], nb["view"], mono, nb["median_depth"]):
            n_matches[k] = -1
            searched.append(np.full(nA, -1, np.int32))
            continue
        nm, mA = search(A["keys"], A["desc"], A["u_right"], has, A["groups"], nb["keys"], nb["desc"], nb["u_right"], nb["has_mp"],
                        nb["groups"], nb["epipolar"], only_stereo, check_orientation)
        searched.append(mA.copy())
        n_matches[k] = nm
        args = (A["view"], nb["view"], A["keys"], A["u_right"], A["depth"], nb["keys"], nb["u_right"], nb["depth"], mA)
        r32, r64 = triangulate(*args, "R32"), triangulate(*args, "R64")
        p = pack_points(r32)
        if device_points is not None:
            loose = ~r64["parity"]
            adopted += int(loose.sum())
            p[loose] = device_points[k][loose]
        pts[k] = p
        n_new[k] = int((p["code"] == OK).sum())
        has[p["code"] == OK] = 1
    return pts, n_matches, n_new, has, adopted, searched


def true_matches(scene, k):
    """matchA of neighbour k from the scene's own correspondences: the row of neighbour k that shows the point of pKF1's row i"""
    inv = np.argsort(scene["neighbors"][k]["order"])
    return inv[scene["A"]["order"]].astype(np.int32)


# ---- the criteria an implementation is held to, shared by the CPU suite (host build of the arithmetic) and the GPU suite -------------
def ulps(got, want, scale):
    """|got - want| in float ulps of `scale`"""
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / np.spacing(np.abs(scale).astype(np.float32)).astype(np.float64)


def check_against_yardstick(name, s, r64, r32, got):
    """The criteria of the GPU suite for one case: `got` are orbfe_new_point records.  Prints every figure before it asserts."""
    par = r64["parity"]
    assert (~par).sum() <= NON_PARITY_CAP * len(par)
    for f in ("code", "path", "idx2"):
        assert np.array_equal(got[f][par], pack_points(r32)[f][par]), f
    ok = par & (r32["code"] == OK)
    rejected = got["code"] != OK
    assert not got["pos"][rejected].any() and not got["normal"][rejected].any() and not got["max_distance"][rejected].any()
    un = ok & (r32["path"] >= PATH_UNPROJECT1)
    if un.any():                                                        # a 3-term product plus an add: 4 ulps of the largest component
        u = ulps(got["pos"][un], r32["pos"][un], np.abs(r32["pos"][un]).max(1, keepdims=True)).max()
        print(f"{name}: {un.sum()} unprojected points within {u:.2f} ulps of R32")
        assert u <= 4
    if ok.any():
        un_, ux, um = (ulps(got["normal"][ok], r32["normal"][ok], np.abs(r32["normal"][ok]).max(1, keepdims=True)).max(),
                       ulps(got["max_distance"][ok], r32["max_distance"][ok], r32["max_distance"][ok]).max(),
                       ulps(got["min_distance"][ok], r32["min_distance"][ok], r32["min_distance"][ok]).max())
        print(f"{name}: {ok.sum()} accepted: normal {un_:.2f}, max_distance {ux:.2f}, min_distance {um:.2f} ulps of R32")
        assert un_ <= 4 and ux <= 4 and um <= 4
    lin = ok & (r32["path"] == PATH_LINEAR)
    if lin.any():
        # both sides of the criterion come from the yardstick: the float reading's own error against the truth
        e32, eg = rel_error(r32["pos"][lin], r64["pos"][lin]), rel_error(got["pos"][lin], r64["pos"][lin])
        ulp = 2.0 ** -23
        print(f"{name}: {lin.sum()} linear points: e(R32) median {np.median(e32):.3g} max {e32.max():.3g}; e(got) median "
              f"{np.median(eg):.3g} max {eg.max():.3g}; ratios {np.median(eg) / np.median(e32):.3f} {eg.max() / e32.max():.3f}")
        assert np.median(eg) <= 4 * np.median(e32) + 2 * ulp and eg.max() <= 4 * e32.max() + 2 * ulp


def scene_args(s):
    mono = s.get("mono", False)
    return (s["view1"], s["keys1"], None if mono else s["ur1"], None if mono else s["depth1"], s["view2"], s["keys2"],
            None if mono else s["ur2"], None if mono else s["depth2"], s["matchA"])
