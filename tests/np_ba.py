"""A float64 numpy reading of Optimizer::BundleAdjustment (L/src/Optimizer.cc:52-231) from the edge list on, and a plain float32
reading of what Tracking::CreateInitialMapMonocular does around it (L/src/Tracking.cc:584-642, KeyFrame::ComputeSceneMedianDepth,
L/src/KeyFrame.cc:588-615): the yardstick of tests/test_ba_cpu.py and tests/test_ba_gpu.py.

What g2o does with an edge list is tests/np_lba.py's reading and is imported, not copied: the problem with its errors and Jacobians
(_Problem), the two solves of a trial (_solve_schur, _solve_full) and the Huber columns.  The loop is this file's own, because the
schedule differs: ONE optimize(n) over every edge, the Huber kernel on all edges or on none, no classification, no second round.
Two things differ from LocalBundleAdjustment beyond the schedule, both read off the source:
  * the monocular Huber delta is (float)sqrt(5.99) (:82), not (float)sqrt(5.991); the stereo delta is (float)sqrt(7.815) in both.
    Five robust iterations therefore equal round 1 of np_lba.optimize wherever no monocular edge reaches its Huber branch in either
    (an all-stereo scene, for one), and np_ba.optimize(..., delta_mono=np_lba.DELTA_MONO) equals it everywhere;
  * EVERY keyframe's estimate is written back through Converter::toCvMat(SE3Quat) (:189-203), the fixed one's too.
A point without an edge is removed from the graph (:175-180) and keeps its float position.  Everything is double; inputs are the
floats the ABI carries, widened.  A reading, unpinned."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import np_lba as Q
from tests import np_pose as NP
from tests.np_lba import EDGE_DTYPE, _huber_cols, _Problem, _solve_full, _solve_schur   # noqa: F401

F32 = np.float32


def worst_ratio(poses, points, ref_poses, ref_points):
    """np_lba.worst_ratio with NaN == NaN: a NaN must stand where the reading has one (else infinity), and counts as no difference"""
    got = [np.asarray(a, np.float64).reshape(-1) for a in (poses, points)]
    ref = [np.asarray(a, np.float64).reshape(-1) for a in (ref_poses, ref_points)]
    for g, r in zip(got, ref):
        if not np.array_equal(np.isnan(g), np.isnan(r)):
            return math.inf
    clean = lambda a: np.where(np.isnan(a), 0.0, a)
    return Q.worst_ratio(clean(got[0]), clean(got[1]), clean(ref[0]), clean(ref[1]))


DELTA_MONO = float(F32(math.sqrt(5.99)))       # Optimizer.cc:82 (const float)
DELTA_STEREO = float(F32(math.sqrt(7.815)))    # :83


def optimize(poses, fixed, points, edges, cam, n_iterations=5, robust=True, solve="schur", order_seed=None, noise=0.0,
             delta_mono=DELTA_MONO):
    """BundleAdjustment from the edge list on; arguments as np_lba.optimize's, fixed: mnId == 0.  Returns a dict: poses [n_kf, 12]
    float32, points [n_pt, 3] float32, rounds (1, or 0 without a free keyframe or an edge), iterations, trials, chi2_first,
    chi2_final, accepts (one boolean per trial)."""
    poses = np.asarray(poses, F32).reshape(-1, 12)
    points = np.asarray(points, F32).reshape(-1, 3)
    edges = np.asarray(edges, EDGE_DTYPE).reshape(-1)
    P = _Problem(poses, fixed, points, edges, cam)
    P.delta = np.where(P.stereo, DELTA_STEREO, delta_mono)
    res = dict(poses=poses.copy(), points=points.copy(), rounds=0, iterations=0, trials=0, chi2_first=0.0, chi2_final=0.0, accepts=[])
    if P.fixed.all() or P.n_e == 0:
        return res
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    sel = rng.permutation(P.n_e) if rng is not None else np.arange(P.n_e)      # the edges in summation order
    kf_act = np.zeros(P.n_kf, bool)
    kf_act[P.kf] = True
    kf_act &= ~P.fixed
    pt_act = np.zeros(P.n_pt, bool)
    pt_act[P.pt] = True
    akf, apt = np.flatnonzero(kf_act), np.flatnonzero(pt_act)                  # the active vertices: poses first, then points
    slot = np.full(P.n_kf, -1)
    slot[akf] = np.arange(len(akf))
    pslot = np.full(P.n_pt, -1)
    pslot[apt] = np.arange(len(apt))

    def robust_chi(chi2):
        c = (_huber_cols(chi2, P.delta)[0] if robust else chi2)[sel]
        if noise:
            c = c * (1.0 + noise * rng.standard_normal(c.shape))
        return float(np.cumsum(c)[-1])

    lam, ni = 0.0, 2.0
    current_chi = 0.0
    for it in range(n_iterations):
        e, chi2, cam_pt = P.errors()
        current_chi = robust_chi(chi2)
        if it == 0:
            res["chi2_first"] = current_chi
        A, B = P.jacobians(cam_pt)
        rho1 = _huber_cols(chi2, P.delta)[1] if robust else np.ones(P.n_e)
        ow = rho1 * P.w
        we = (-(P.w[:, None] * e)) * rho1[:, None]
        AtO, BtO = A * ow[:, None, None], B * ow[:, None, None]
        blocks = []
        for L_, R_ in ((AtO, A), (BtO, B)):                                    # Hll, Hpp per edge: rows summed in index order
            H_e = np.einsum("nra,nrb->nrab", L_, R_)
            blocks.append((H_e[:, 0] + H_e[:, 1]) + H_e[:, 2])
        Hll_e, Hpp_e = blocks
        Hpl_e = np.einsum("nrb,nra->nrba", B, AtO)                             # [pose row, point column]
        Hpl_e = (Hpl_e[:, 0] + Hpl_e[:, 1]) + Hpl_e[:, 2]
        bl_e = (A[:, 0, :] * we[:, 0:1] + A[:, 1, :] * we[:, 1:2]) + A[:, 2, :] * we[:, 2:3]
        bp_e = (B[:, 0, :] * we[:, 0:1] + B[:, 1, :] * we[:, 1:2]) + B[:, 2, :] * we[:, 2:3]
        if noise:
            for a in (Hll_e, Hpp_e, Hpl_e, bl_e, bp_e):
                a *= 1.0 + noise * rng.standard_normal(a.shape)
        Hpp, bp = np.zeros((len(akf), 6, 6)), np.zeros((len(akf), 6))
        Hll, bl = np.zeros((len(apt), 3, 3)), np.zeros((len(apt), 3))
        Hpl = {}                                                               # (pose slot, point slot) -> 6 x 3
        for i in sel:
            l, s = pslot[P.pt[i]], slot[P.kf[i]]
            Hll[l] += Hll_e[i]
            bl[l] += bl_e[i]
            if s >= 0:
                Hpp[s] += Hpp_e[i]
                bp[s] += bp_e[i]
                Hpl[(s, l)] = Hpl[(s, l)] + Hpl_e[i] if (s, l) in Hpl else Hpl_e[i].copy()
        by_point = [[] for _ in apt]
        for (s, l) in sorted(Hpl):
            by_point[l].append(s)
        if it == 0:                                                            # computeLambdaInit over every active vertex
            # A NaN entry of the diagonal does not enter the maximum, as in np_lba.optimize and in the library (fmax).  g2o's
            # std::max(fabs(h), maxDiagonal) would let it REPLACE the running maximum until the next entry: a value that depends on
            # which vertex comes last, not a rule; defined here where the reference is not
            md = 0.0
            for h in list(Hpp) + list(Hll):
                for d in np.abs(np.diag(h)):
                    md = max(md, float(d))                                     # max(md, NaN) is md
            lam, ni = 1e-5 * md, 2.0
        rho, qmax = 0.0, 0
        while True:
            res["trials"] += 1
            ok2, xp, xl = _solve_schur(Hpp, bp, Hll, bl, Hpl, by_point, lam) if solve == "schur" else _solve_full(Hpp, bp, Hll, bl, Hpl, lam)
            saved = P.Q.copy(), P.T.copy(), P.X.copy()                         # push
            if ok2:
                for s, k in enumerate(akf):
                    P.Q[k], P.T[k] = NP.se3_mul(NP.se3_exp(xp[6 * s:6 * s + 6]), (list(P.Q[k]), list(P.T[k])))
                P.X[apt] += xl.reshape(-1, 3)
                temp_chi = robust_chi(P.errors()[1])
                scale = 0.0
                xs, bs = np.concatenate([xp, xl]), np.concatenate([bp.reshape(-1), bl.reshape(-1)])
                for j in range(len(xs)):
                    scale += xs[j] * (lam * xs[j] + bs[j])                     # computeScale over the whole vector
                scale += 1e-3
            else:
                temp_chi, scale = float(np.finfo(np.float64).max), 1.0
            with np.errstate(all="ignore"):
                rho = float((np.float64(current_chi) - np.float64(temp_chi)) / np.float64(scale))
            good = rho > 0 and math.isfinite(temp_chi) and ok2
            res["accepts"].append(bool(good))
            if good:
                alpha = 1.0 - math.pow(2 * rho - 1, 3) if abs(rho) < 1e100 else -math.inf
                lam *= max(1.0 / 3.0, min(alpha, 2.0 / 3.0))
                ni = 2.0
                current_chi = temp_chi
            else:
                lam *= ni
                ni *= 2
                P.Q, P.T, P.X = saved                                          # pop
                if not math.isfinite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        res["iterations"] += 1
        if qmax == 10 or rho == 0 or not math.isfinite(lam):
            break
    res["chi2_final"], res["rounds"] = current_chi, 1
    res["poses"] = np.stack([NP.se3_to_Tcw((list(P.Q[k]), list(P.T[k]))) for k in range(P.n_kf)]).astype(F32)
    pts = points.copy()
    pts[pt_act] = P.X[pt_act].astype(F32)
    res["points"] = pts
    return res


# ---- the adjustment's cases --------------------------------------------------------------------------------------------------------
def exact_scene(n_points=12):
    """A scene AT its optimum in exact arithmetic: identity rotations, integer translations along z, points with small integer x, y and a
    power of two for the depth in every keyframe, fx = fy = 512 -- every projection is a float, every error is exactly 0.  The first
    trial's step is exactly 0, rho = 0 / 1e-3 = 0 and optimize() terminates after ONE iteration (levenberg.cpp: rho == 0), whatever
    n_iterations asks for and whatever the summation order: the one early termination that is decided by more than rounding noise."""
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0, mbf=64.0)
    n_kf = 3
    poses = np.zeros((n_kf, 12), F32)
    poses[:, [0, 5, 10]] = 1.0
    poses[:, 11] = [0.0, 8.0, 24.0]                                            # depths 8, 16, 32
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = 1
    points = np.array([[(p % 5) - 2, (p // 5) - 1, 8.0] for p in range(n_points)], F32)
    rows = []
    for p, X in enumerate(points):
        for k in range(n_kf):
            z = float(X[2] + poses[k, 11])
            u, v = float(X[0]) / z * cam["fx"] + cam["cx"], float(X[1]) / z * cam["fy"] + cam["cy"]
            rows.append((k, p, u, v, -1.0 if (p + k) % 2 else u - cam["mbf"] / z, 1.0))
    return dict(poses=poses, fixed=fixed, points=points, edges=np.array(rows, EDGE_DTYPE), cam=cam)


def make_scene(seed, lonely_point=False, lonely_kf=False, **kw):
    """np_lba.make_scene with the keyframes BundleAdjustment fixes: n_fixed = 1 puts keyframe 0 (mnId == 0, the identity pose) into the
    map, n_fixed = 0 leaves it out (nothing is fixed).  lonely_point: one more point, far away, that no keyframe observes;
    lonely_kf: one more free keyframe that observes nothing."""
    kw.setdefault("n_fixed", 1)
    s = Q.make_scene(seed, **kw)
    if lonely_point:
        s["points"] = np.concatenate([s["points"], np.array([[1234.5, -6.25, 77.0]], F32)])
    if lonely_kf:
        extra = s["poses"][-1:].copy()
        extra[0, 3] += 0.37
        s["poses"], s["fixed"] = np.concatenate([s["poses"], extra]), np.concatenate([s["fixed"], np.zeros(1, np.uint8)])
        s["poses_true"] = np.concatenate([s["poses_true"], extra])
    return s


@functools.lru_cache(maxsize=None)
def stereo_scene():
    """the scene on which five robust iterations ARE round 1 of LocalBundleAdjustment: no monocular edge (the deltas agree), and the
    one fixed keyframe is the identity, which the quaternion gives back exactly"""
    s = make_scene(500, n_free=4, n_points=150, mono=0.0, u_min=300)
    s["n_iterations"], s["robust"], s["flags"] = 5, True, Q.FIRST_ROUND_ONLY
    return s


# name -> (seed or None for exact_scene, keyword arguments of make_scene, n_iterations, robust).  Seeds: the first ones tried, from the
# case's number in the table x 100 on, for which the conditions of tests/test_ba_cpu.py hold (what the name promises, equal accepts in
# every run, half the parity tolerance between the runs).
CASES = {
    "robust_5": (100, dict(n_free=5, n_points=200), 5, True),
    "plain_10": (200, dict(n_free=5, n_points=200), 10, False),
    "robust_1": (300, dict(n_free=3, n_points=120), 1, True),
    "robust_20": (400, dict(n_free=3, n_points=150), 20, True),
    "plain_5_mono": (500, dict(n_free=4, n_points=150, mono=1.0), 5, False),
    "robust_10_stereo": (600, dict(n_free=4, n_points=150, mono=0.0, u_min=300), 10, True),
    "rejected_step": (701, dict(n_free=4, n_points=150, rot=0.4, trans=3.0, point_noise=3.0), 10, True),
    "at_optimum": (None, dict(), 20, True),
    "nothing_fixed": (900, dict(n_free=4, n_fixed=0, n_points=150), 5, True),
    "lonely_point": (1000, dict(n_free=2, n_points=60, lonely_point=True), 5, True),
    "lonely_keyframe": (1100, dict(n_free=2, n_points=60, lonely_kf=True), 5, False),
    "two_keyframes": (1200, dict(n_free=1, n_points=100, mono=1.0), 10, True),
    "nine_keyframes": (1300, dict(n_free=8, n_points=300), 5, True),
    "points_255": (1400, dict(n_free=2, n_points=255, outliers=0.0), 5, True),
    "points_256": (1400, dict(n_free=2, n_points=256, outliers=0.0), 5, True),
    "points_257": (1400, dict(n_free=2, n_points=257, outliers=0.0), 5, True),
    "edges_0": (1500, dict(n_free=2, n_points=0), 5, True),
    "no_free": (1600, dict(n_free=0, n_points=20), 5, True),
}


@functools.lru_cache(maxsize=None)
def case_scene(name):
    seed, kw, n_it, robust = CASES[name]
    s = exact_scene() if seed is None else make_scene(seed, **kw)
    s["n_iterations"], s["robust"] = n_it, robust
    return s


def run_scene(s, **kw):
    kw.setdefault("n_iterations", s["n_iterations"])
    kw.setdefault("robust", s["robust"])
    return optimize(s["poses"], s["fixed"], s["points"], s["edges"], s["cam"], **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reading of a case, computed once and shared; treat it as read-only"""
    return run_scene(case_scene(name))


# ---- Tracking::CreateInitialMapMonocular around the adjustment, in float32 ---------------------------------------------------------------
MAP_MEDIAN_NEGATIVE, MAP_FEW_POINTS, MAP_NO_POINTS = 1, 2, 4               # the reason bits of orbfe_initial_map_result
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)


def build_map(keys1, keys2, matches12, P3D, triangulated, R21, t21, octaves1, octaves2, inv_level_sigma2, pose1=None):
    """Tracking.cc:551-556, :584-612: the matches that were triangulated, in order of i, as points with two monocular observations
    each.  Returns (index list, poses [2, 12], fixed, points, edges)."""
    keys1, keys2 = np.asarray(keys1, F32).reshape(-1, 2), np.asarray(keys2, F32).reshape(-1, 2)
    m = np.asarray(matches12, np.int64).reshape(-1)
    tri = np.asarray(triangulated, bool).reshape(-1)
    sig = np.asarray(inv_level_sigma2, F32).reshape(-1)
    idx = np.flatnonzero((m >= 0) & (m < len(keys2)) & tri[:len(m)])
    rows = []
    for p, i in enumerate(idx):
        rows.append((0, p, keys1[i, 0], keys1[i, 1], -1.0, sig[octaves1[i]]))
        rows.append((1, p, keys2[m[i], 0], keys2[m[i], 1], -1.0, sig[octaves2[m[i]]]))
    edges = np.array(rows, EDGE_DTYPE) if rows else np.zeros(0, EDGE_DTYPE)
    pose2 = np.concatenate([np.asarray(R21, F32).reshape(3, 3), np.asarray(t21, F32).reshape(3, 1)], 1).reshape(12)
    poses = np.stack([IDENTITY if pose1 is None else np.asarray(pose1, F32).reshape(12), pose2]).astype(F32)
    return idx.astype(np.int32), poses, np.array([1, 0], np.uint8), np.asarray(P3D, F32).reshape(-1, 3)[idx], edges


def scene_depths(pose1, points):
    """ComputeSceneMedianDepth's vDepths: float z = Rcw2.dot(x3Dw) + zcw, cv::Mat::dot accumulating in double in element order (this
    project's restatement), the sum with zcw in double, rounded to float once"""
    T = np.asarray(pose1, F32).reshape(3, 4).astype(np.float64)
    X = np.asarray(points, F32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        s = ((0.0 + T[2, 0] * X[:, 0]) + T[2, 1] * X[:, 1]) + T[2, 2] * X[:, 2]
        return (s + T[2, 3]).astype(F32)


def depth_keys(z):
    """a float depth as an unsigned key of the same order, the order the library sorts by: -0 before +0, NaN (on which std::sort is
    undefined) last"""
    z = np.asarray(z, F32)
    b = z.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(z), np.uint32(0xFFFFFFFF), k)


def finish_map(poses, points, matches_of_points, q=2, min_points=100):
    """Tracking.cc:620-642 on the adjustment's outputs: the median depth in the initial keyframe, both reset conditions, the rescale in
    float.  The depths are sorted by depth_keys: where std::sort is free (equal depths, -0 against +0) or undefined (NaN) the order is
    the library's.  matches_of_points: the keypoint of frame 2 every point is observed at -- pKFcur->TrackedMapPoints(1) counts the
    keypoints that hold a point.  Returns a dict: poses, points (scaled iff success), median_depth, tracked, reason, success, depths,
    n_points."""
    poses, points = np.asarray(poses, F32).reshape(2, 12).copy(), np.asarray(points, F32).reshape(-1, 3).copy()
    n = len(points)
    z = scene_depths(poses[0], points)
    zs = z[np.argsort(depth_keys(z), kind="stable")]
    median = F32(zs[(n - 1) // q]) if n else F32(0)
    tracked = len(set(np.asarray(matches_of_points).reshape(-1).tolist()))
    reason = MAP_NO_POINTS if n == 0 else 0
    reason |= MAP_MEDIAN_NEGATIVE if median < 0 else 0
    reason |= MAP_FEW_POINTS if tracked < min_points else 0
    out = dict(median_depth=median, tracked=tracked, reason=reason, success=reason == 0, depths=z, n_points=n)
    if reason == 0:
        with np.errstate(all="ignore"):
            inv = F32(1.0) / median
            poses[1, [3, 7, 11]] = poses[1, [3, 7, 11]] * inv
            points = points * inv
    out["poses"], out["points"] = poses, points
    return out


def create_initial_map(keys1, keys2, matches12, P3D, triangulated, R21, t21, octaves1, octaves2, inv_level_sigma2, cam, n_iterations=20,
                       q=2, min_points=100, pose1=None, **kw):
    """CreateInitialMapMonocular from the initialiser's outputs to the scaled map.  Returns finish_map's dict with index (the
    compacted list), ba (optimize's dict), unscaled_poses / unscaled_points (the adjustment's outputs), points_full [n1, 3] in
    match-index order with zero rows where there is no point."""
    idx, poses, fixed, points, edges = build_map(keys1, keys2, matches12, P3D, triangulated, R21, t21, octaves1, octaves2,
                                                 inv_level_sigma2, pose1)
    ba = optimize(poses, fixed, points, edges, cam, n_iterations=n_iterations, robust=True, **kw)
    out = finish_map(ba["poses"], ba["points"], np.asarray(matches12).reshape(-1)[idx], q, min_points)
    full = np.zeros((len(np.asarray(matches12).reshape(-1)), 3), F32)
    full[idx] = out["points"]
    out.update(index=idx, ba=ba, unscaled_poses=ba["poses"], unscaled_points=ba["points"], points_full=full, edges=edges)
    return out


def two_view_scene(seed, N=300, n_extra=40, noise=0.3, n_levels=8, scale_factor=1.2, drop=0.1, **kw):
    """tests/np_initializer.py's seeded two-view scene carried to where CreateInitialMapMonocular starts: its keypoints and matches,
    the true motion (unit baseline) rounded to float as R21 / t21, P3D = the true points at that scale plus 2 % noise, a share `drop`
    of the matches not triangulated, octaves drawn per keypoint, the pyramid's inv_level_sigma2."""
    from tests import np_initializer as I
    keys1, keys2, m12, params, truth = I.scene(seed, "general", N=N, n_extra=n_extra, noise=noise, **kw)
    rng = np.random.default_rng(seed + 7)
    fx, fy, cx, cy = params[:4]
    n1, n2 = len(keys1), len(keys2)
    # the scene's own points are not handed out: triangulate the noise-free geometry again from keys1 and the true motion
    R, t = truth["R"], truth["t"]
    i1 = np.flatnonzero(m12 >= 0)
    a = np.stack([(keys1[i1, 0] - cx) / fx, (keys1[i1, 1] - cy) / fy, np.ones(len(i1))], 1)
    b = np.stack([(keys2[m12[i1], 0] - cx) / fx, (keys2[m12[i1], 1] - cy) / fy, np.ones(len(i1))], 1)
    P3D = np.zeros((n1, 3), F32)
    for k, i in enumerate(i1):                                                 # depth along ray a from the two-ray midpoint equations
        M = np.stack([R @ a[k], -b[k]], 1)
        d = np.linalg.lstsq(M, -t, rcond=None)[0]
        P3D[i] = (a[k] * d[0] * (1.0 + 0.02 * rng.normal())).astype(F32)
    tri = np.zeros(n1, bool)
    tri[i1] = rng.uniform(size=len(i1)) >= drop
    P3D[~tri] = 0
    sig = np.array([1.0 / (scale_factor ** l) ** 2 for l in range(n_levels)], F32)
    return dict(keys1=keys1, keys2=keys2, matches12=m12, P3D=P3D, triangulated=tri, R21=R.astype(F32), t21=t.astype(F32),
                octaves1=rng.integers(0, n_levels, n1).astype(np.int32), octaves2=rng.integers(0, n_levels, n2).astype(np.int32),
                inv_level_sigma2=sig, cam=dict(fx=fx, fy=fy, cx=cx, cy=cy, mbf=0.0))


def run_map(s, **kw):
    return create_initial_map(s["keys1"], s["keys2"], s["matches12"], s["P3D"], s["triangulated"], s["R21"], s["t21"], s["octaves1"],
                              s["octaves2"], s["inv_level_sigma2"], s["cam"], **kw)


def exact_two_view(depths, min_levels=2, duplicate=False, unmatched=3):
    """A two-view map AT its optimum in exact arithmetic (see exact_scene): the adjustment terminates after one iteration and leaves
    every point where P3D put it, so the finish stage sees hand-placed depths -- ties, signs, a NaN.  depths: one per point, powers of
    two (negative ones allowed; NaN makes the adjustment a no-op of another kind: every trial is rejected).  The current keyframe
    stands one unit to the right.  `unmatched` keypoints without a match are interleaved; duplicate: the last two points share
    their keypoint in frame 2."""
    n = len(depths)
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0, mbf=0.0)
    X = np.array([[(k % 7) - 3, (k // 7) % 5 - 2, z] for k, z in enumerate(depths)], np.float64)
    n1 = n + unmatched
    slots = np.array([k + min(k // 2, unmatched) for k in range(n)])          # where the matched keypoints sit in frame 1
    keys1 = np.full((n1, 2), 7.0, F32)
    keys2 = np.full((n + 1, 2), 9.0, F32)
    m12 = np.full(n1, -1, np.int32)
    P3D = np.zeros((n1, 3), F32)
    tri = np.zeros(n1, bool)
    for k in range(n):
        z = X[k, 2] if np.isfinite(X[k, 2]) else 8.0
        j = n - 1 - k if not (duplicate and k == n - 1) else 1               # frame 2 lists them backwards
        keys1[slots[k]] = (X[k, 0] / z * 512 + 320, X[k, 1] / z * 512 + 240)
        keys2[j] = ((X[k, 0] - 1) / z * 512 + 320, X[k, 1] / z * 512 + 240)
        m12[slots[k]], P3D[slots[k]], tri[slots[k]] = j, X[k], True
    rng = np.random.default_rng(n)
    return dict(keys1=keys1, keys2=keys2, matches12=m12, P3D=P3D, triangulated=tri, R21=np.eye(3, dtype=F32),
                t21=np.array([-1, 0, 0], F32), octaves1=rng.integers(0, min_levels, n1).astype(np.int32),
                octaves2=rng.integers(0, min_levels, n + 1).astype(np.int32), inv_level_sigma2=np.array([1.0, 0.25], F32), cam=cam)


def general_pose(s, seed=5):
    """the scene s seen from a world frame in which the initial keyframe has a general pose: pose1 = [R1 | t1], the current keyframe
    [R21 R1 | R21 t1 + t21], P3D moved along; everything rounded to float once more"""
    rng = np.random.default_rng(seed)
    R1, t1 = NP.rodrigues(rng.normal(size=3) * 0.3), rng.normal(size=3)
    out = dict(s)
    R21, t21 = s["R21"].astype(np.float64), s["t21"].astype(np.float64)
    out["pose1"] = np.concatenate([R1, t1[:, None]], 1).reshape(12).astype(F32)
    out["R21"], out["t21"] = (R21 @ R1).astype(F32), (R21 @ t1 + t21).astype(F32)
    P = (s["P3D"].astype(np.float64) - t1) @ R1
    out["P3D"] = np.where(s["triangulated"][:, None], P, 0.0).astype(F32)
    return out


def mirrored(s, share=0.6, seed=9):
    """the scene with a share of its points placed BEHIND the initial keyframe, at the mirror image through its centre (the same
    pixel in frame 1): the hand-placed P3D of a negative median"""
    rng = np.random.default_rng(seed)
    out = dict(s)
    flip = s["triangulated"] & (rng.uniform(size=len(s["P3D"])) < share)
    out["P3D"] = np.where(flip[:, None], -s["P3D"], s["P3D"]).astype(F32)
    return out


def _two_view(seed, **kw):
    """the scenes of the adjustment's cases: 5 % of the matches are wrong and the keypoints carry 0.6 px of noise.  On a scene without
    wrong matches the 20 iterations converge to the last bit half-way and every later accept / reject is rounding noise: no parity case"""
    return two_view_scene(seed, outliers=0.05, noise=0.6, **kw)


# name -> builder of the scene, keyword arguments of create_initial_map.  tri_N: N matches, all triangulated, around min_points = 100;
# n1_K: K keypoints in frame 1 (the word boundaries of the build stage); even / odd: (n - 1) / 2 of 6 and 7 hand-placed depths.
# Seeds: the first ones tried, from the case's number in the table x 10 on, for which the conditions of tests/test_ba_cpu.py hold
# (equal accepts and the same reset decision in every run, half the parity tolerance between the runs).
MAP_CASES = {
    "typical": (lambda: _two_view(315, N=300), {}),
    "tri_99": (lambda: _two_view(321, N=99, drop=0.0), {}),
    "tri_100": (lambda: _two_view(333, N=100, drop=0.0), {}),
    "tri_101": (lambda: _two_view(340, N=101, drop=0.0), {}),
    "n1_63": (lambda: _two_view(350, N=50, n_extra=13), dict(min_points=20)),
    "n1_64": (lambda: _two_view(360, N=50, n_extra=14), dict(min_points=20)),
    "n1_65": (lambda: _two_view(370, N=50, n_extra=15), dict(min_points=20)),
    "n1_128": (lambda: _two_view(382, N=100, n_extra=28), dict(min_points=20)),
    "n1_129": (lambda: _two_view(390, N=100, n_extra=29), dict(min_points=20)),
    "even": (lambda: exact_two_view([4.0, 16.0, 2.0, 8.0, 32.0, 64.0]), dict(min_points=3)),
    "odd": (lambda: exact_two_view([4.0, 16.0, 2.0, 8.0, 32.0, 64.0, 1.0]), dict(min_points=3)),
    "ties": (lambda: exact_two_view([8.0, 4.0, 8.0, 8.0, 16.0, 8.0, 2.0, 8.0]), dict(min_points=3)),
    "duplicate_keypoint": (lambda: exact_two_view([8.0, 4.0, 2.0, 16.0, 8.0], duplicate=True), dict(min_points=5)),
    "exact_negative": (lambda: exact_two_view([-8.0, 4.0, -2.0, -16.0, 8.0]), dict(min_points=3)),
    "nan_depth": (lambda: exact_two_view([8.0, float("nan"), 2.0, 16.0, 4.0]), dict(min_points=3)),
    "negative_median": (lambda: mirrored(_two_view(400, N=150, drop=0.0)), {}),
    "zero_points": (lambda: _two_view(410, N=120, drop=1.0), {}),
    "general_pose": (lambda: general_pose(_two_view(420, N=150)), {}),
    "q_3": (lambda: _two_view(430, N=120), dict(q=3, min_points=50, n_iterations=10)),
}


@functools.lru_cache(maxsize=None)
def map_scene(name):
    build, kw = MAP_CASES[name]
    s = build()
    s["kw"] = dict(kw)
    return s


def run_map_case(s, **more):
    kw = dict(s["kw"])
    kw.update(more)
    if "pose1" in s:
        kw["pose1"] = s["pose1"]
    return run_map({k: v for k, v in s.items() if k not in ("kw", "pose1")}, **kw)


@functools.lru_cache(maxsize=None)
def map_reference(name):
    """the reading of a map case, computed once and shared; treat it as read-only"""
    return run_map_case(map_scene(name))
