"""A numpy reading of Sim3Solver (L/src/Sim3Solver.cc, L/ = Source/Libraries/ORB_SLAM2/): the constructor's preparation (:85-107),
ComputeSim3 (:216-322) and CheckInliers (:324-344) for all hypotheses of a problem at once, plus the acceptance rule of iterate
(:178-199).  The yardstick of tests/test_sim3_cpu.py and tests/test_sim3_gpu.py.  Written from the reference's source, not from
csrc/sim3_internal.h, and structured differently on purpose: every step is an array over (hypothesis, ...), the eigenvector is
LAPACK's (numpy.linalg.eigh), the rotation is I + sin(a) K + (1 - cos(a)) K^2.

Two modes:
  R64  every operation in float64 on the float32 inputs.  The truth.
  R32  float32 where the reference is float (camera-frame points, projections, centroids, Pr, M, P3, errors), float64 where it is
       double (the sums of N, ang, nom / den, Mat::dot), eigh on the float32 matrix = LAPACK's single-precision driver.  It stands in
       for the reference's float result and shows what that precision does by itself.

Margin verdicts (R64).  A hypothesis is a PARITY hypothesis when the gap between its two largest eigenvalues is at least EIG_GAP
relative to the largest, the norm of its quaternion's imaginary part is at least IMAG_TINY and, for a free scale, sqrt(den) is at least
DEN_TINY times the largest coordinate of the triple (Pr carries the float rounding of the uncentred coordinates).  A (hypothesis,
correspondence) decision is a PARITY decision when the hypothesis is one and both errors are at least ERR_MARGIN x bound away from
their bounds.  Only those can be compared bit for bit between implementations whose eigen-solver, atan2 and sin / cos differ."""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
EIG_GAP, ERR_MARGIN, IMAG_TINY, DEN_TINY = 1e-3, 1e-2, 1e-5, 1e-3
NON_PARITY_CAP = 0.03     # of a case's decisions, and of its hypotheses
MIN_INLIERS = 20          # LoopClosing.cc:263: SetRansacParameters(0.99, 20, 300)

VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
PAIR_DTYPE = np.dtype([("Xw1", "<f4", (3,)), ("Xw2", "<f4", (3,)), ("max_err1", "<f4"), ("max_err2", "<f4")])
KITTI = dict(fx=718.856, fy=718.856, cx=607.19, cy=185.2, mb=0.537)


def make_view(R, t, cam=KITTI):
    v = np.zeros(1, VIEW_DTYPE)
    v["Rcw"][0], v["tcw"][0] = np.asarray(R, F64).astype(F32).reshape(9), np.asarray(t, F64).astype(F32)
    v["fx"], v["fy"], v["cx"], v["cy"] = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    return v


def _rows(A, x):
    """(A x) for a 3 x 3 (or (H, 3, 3)) A and x[..., 3] in the working type: a dot of three products in index order"""
    return np.stack([A[..., r, 0] * x[..., 0] + A[..., r, 1] * x[..., 1] + A[..., r, 2] * x[..., 2] for r in range(3)], -1)


def _image(v, c, T):
    invz = T(1) / c[..., 2]
    return np.stack([T(v["fx"]) * (c[..., 0] * invz) + T(v["cx"]), T(v["fy"]) * (c[..., 1] * invz) + T(v["cy"])], -1)


def prepare(view1, view2, pairs, mode):
    """:92-96 and FromCameraToImage: camera-frame points and their own projections, (n, 3) and (n, 2) each"""
    T = F64 if mode == "R64" else F32
    v1, v2 = np.asarray(view1).reshape(-1)[0], np.asarray(view2).reshape(-1)[0]
    out = []
    for v, X in ((v1, pairs["Xw1"]), (v2, pairs["Xw2"])):
        c = _rows(v["Rcw"].astype(T).reshape(3, 3), X.astype(T)) + v["tcw"].astype(T)
        out += [c, _image(v, c, T)]
    return out[0], out[2], out[1], out[3]           # c1, c2, im1, im2


def solve(view1, view2, pairs, triples, fix_scale, mode="R64"):
    """All hypotheses of one problem.  Returns a dict: s (H), R (H,3,3), t (H,3), inl (H,n) bool, count (H), err1 / err2 (H,n), and in
    R64 also gap, imag, parity_h (H) and parity (H,n)."""
    assert mode in ("R64", "R32")
    T = F64 if mode == "R64" else F32
    v1, v2 = np.asarray(view1).reshape(-1)[0], np.asarray(view2).reshape(-1)[0]
    tr = np.asarray(triples, np.int64).reshape(-1, 3)
    H, n = len(tr), len(pairs)
    with np.errstate(all="ignore"):
        c1, c2, im1, im2 = prepare(view1, view2, pairs, mode)
        P1, P2 = c1[tr], c2[tr]                                            # (H, point, coordinate)
        # Step 1 (:207-214)
        O1 = (P1[:, 0] + P1[:, 1] + P1[:, 2]) * T(1.0 / 3.0)
        O2 = (P2[:, 0] + P2[:, 1] + P2[:, 2]) * T(1.0 / 3.0)
        Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
        # Step 2 (:233): M[i][j] = sum over the points of Pr2[i] * Pr1[j]
        M = np.empty((H, 3, 3), T)
        for i in range(3):
            for j in range(3):
                M[:, i, j] = Pr2[:, 0, i] * Pr1[:, 0, j] + Pr2[:, 1, i] * Pr1[:, 1, j] + Pr2[:, 2, i] * Pr1[:, 2, j]
        # Step 3 (:241-253): double sums, stored in the matrix's type
        m = M.astype(F64)
        N = np.empty((H, 4, 4), F64)
        N[:, 0, 0] = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
        N[:, 0, 1] = m[:, 1, 2] - m[:, 2, 1]
        N[:, 0, 2] = m[:, 2, 0] - m[:, 0, 2]
        N[:, 0, 3] = m[:, 0, 1] - m[:, 1, 0]
        N[:, 1, 1] = m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2]
        N[:, 1, 2] = m[:, 0, 1] + m[:, 1, 0]
        N[:, 1, 3] = m[:, 2, 0] + m[:, 0, 2]
        N[:, 2, 2] = -m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2]
        N[:, 2, 3] = m[:, 1, 2] + m[:, 2, 1]
        N[:, 3, 3] = -m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]
        for i in range(4):
            for j in range(i):
                N[:, i, j] = N[:, j, i]
        N = N.astype(T)
        finite = np.isfinite(N).all((1, 2))
        w, V = np.linalg.eigh(np.where(finite[:, None, None], N, 0))      # ascending: the last column belongs to the largest
        assert V.dtype == T
        q = V[:, :, 3]
        # Step 4 (:261-273)
        vec = q[:, 1:4]
        nv = np.sqrt((vec.astype(F64) ** 2).sum(1))
        ang = np.arctan2(nv, q[:, 0].astype(F64))
        rv = (vec * (2 * ang / nv).astype(T)[:, None]).astype(F64)        # cv::Rodrigues works in double on the float vector
        a = np.sqrt((rv ** 2).sum(1))
        k = rv / a[:, None]
        K = np.zeros((H, 3, 3), F64)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
        R = (np.eye(3) + np.sin(a)[:, None, None] * K + (1 - np.cos(a))[:, None, None] * (K @ K)).astype(T)
        # Step 5 (:277): P3 = R * Pr2, here per point
        P3 = np.stack([_rows(R, Pr2[:, j]) for j in range(3)], 1)
        # Step 6 (:281-296)
        nom = (Pr1.astype(F64) * P3.astype(F64)).sum((1, 2))
        den = (P3 * P3).astype(F64).sum((1, 2))
        s = np.ones(H, T) if fix_scale else (nom / den).astype(T)
        # Step 7 (:301)
        t = O1 - (_rows(R, O2).astype(F64) * s.astype(F64)[:, None]).astype(T)
        # Step 8 (:306-321)
        sR = s[:, None, None] * R
        sRinv = (1.0 / s.astype(F64)).astype(T)[:, None, None] * np.swapaxes(R, 1, 2)
        tinv = -_rows(sRinv, t)
        # CheckInliers (:324-344): (H, n)
        p21 = _image(v1, _rows(sR[:, None], c2[None]) + t[:, None], T)
        p12 = _image(v2, _rows(sRinv[:, None], c1[None]) + tinv[:, None], T)
        d1, d2 = (im1[None] - p21).astype(F64), (p12 - im2[None]).astype(F64)
        err1, err2 = (d1 ** 2).sum(2).astype(T), (d2 ** 2).sum(2).astype(T)
        b1, b2 = pairs["max_err1"].astype(T)[None], pairs["max_err2"].astype(T)[None]
        inl = (err1 < b1) & (err2 < b2)
    res = dict(s=s, R=R, t=t, inl=inl, count=inl.sum(1).astype(np.int32), err1=err1, err2=err2)
    if mode == "R64":
        gap = (w[:, 3] - w[:, 2]) / np.abs(w[:, 3])
        scale = np.abs(P2).max((1, 2))
        par_h = finite & (gap >= EIG_GAP) & (nv >= IMAG_TINY) & np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1)
        if not fix_scale:
            par_h &= np.sqrt(den) >= DEN_TINY * scale
        with np.errstate(all="ignore"):
            clear = (np.abs(err1 - b1) >= ERR_MARGIN * b1) & (np.abs(err2 - b2) >= ERR_MARGIN * b2)
        res.update(gap=gap, imag=nv, parity_h=par_h, parity=par_h[:, None] & clear, Pr1=Pr1, O2=O2)
    return res


def select(counts, min_inliers):
    """(returned, best) of a solver that runs hypotheses 0 .. H-1 in order (:178-193): the first count > min_inliers ends it and is
    the best; otherwise the best is the LAST maximum (`>=` from mnBestInliers = 0)."""
    best, best_count = -1, 0
    for h, c in enumerate(counts):
        if c >= best_count:
            best, best_count = h, int(c)
            if c > min_inliers:
                return h, h
    return -1, best


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def rot(axis, a):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def bounds(octave, n_levels=8, scale=1.2):
    """mvnMaxError (:85-86): 9.210 * mvLevelSigma2[octave] in double, truncated by the vector<size_t>, as the float CheckInliers
    compares with"""
    sf = np.ones(n_levels, F32)
    for i in range(1, n_levels):
        sf[i] = sf[i - 1] * F32(scale)
    return np.floor(9.210 * (sf * sf).astype(F64)[octave]).astype(F32)


CASES = {
    "fixed_stereo": dict(seed=1, fix_scale=True, true_scale=1.0),
    "free_scale": dict(seed=2, fix_scale=False, true_scale=1.31),
    "mostly_outliers": dict(seed=3, fix_scale=True, true_scale=1.0, outliers=0.85, plant=(5, 22, 23, 41, 58)),
    "near_planar": dict(seed=5, fix_scale=False, true_scale=0.8, zr=(19.8, 20.2), yr=1.0),
    "small_rotation": dict(seed=5, fix_scale=True, true_scale=1.0, angle=2e-3, t12=(0.05, 0.01, 0.1)),
    "twelve_levels": dict(seed=6, fix_scale=False, true_scale=1.1, n_levels=12),
}
CASE_N, CASE_H = 130, 64


def make_scene(seed, n=CASE_N, H=CASE_H, fix_scale=True, true_scale=1.0, outliers=0.3, n_levels=8, noise=True, angle=0.2,
               t12=(0.5, 0.1, 1.0), xr=15.0, yr=3.0, zr=(3.0, 60.0), plant=()):
    """Two keyframes of a KITTI camera and n matched map-point pairs.  The points of keyframe 1 are x +-xr, y +-yr, z in zr in its
    camera frame; keyframe 2 sees them through the true similarity c1 = s R12 c2 + t12 (a rotation of `angle` about a tilted axis) and
    carries them in a map of its own (another world pose).  Noise: a pixel x level scale across the ray and half of z^2 / mbf along
    it, in both maps; gross outliers are other points of the scene.  Octave from depth, bounds truncated.  The H triples are random;
    those at the positions `plant` are drawn from the true correspondences only, so that a scene of mostly outliers still has
    hypotheses with inliers."""
    rng = np.random.default_rng(seed)
    cam = KITTI
    R1, t1 = rot([0, 1, 0], 0.1), np.array([1.0, -0.5, 2.0])
    R2, t2 = rot([0.1, 1, 0], -0.4), np.array([-3.0, 0.2, 7.0])
    R12, t12 = rot([0.2, 1.0, 0.1], angle), np.asarray(t12, F64)
    s12 = 1.0 if fix_scale and true_scale == 1.0 else true_scale
    c1 = np.stack([rng.uniform(-xr, xr, n), rng.uniform(-yr, yr, n), rng.uniform(zr[0], zr[1], n)], 1)
    for _ in range(20):                                                     # every point in front of keyframe 2 as well
        c2 = (c1 - t12) @ R12 / s12                                         # R12^T (c1 - t12) / s
        low = c2[:, 2] * s12 < 1.0
        c1[low, 2] += 5.0
    bad = rng.random(n) < (outliers if noise else 0.0)
    c2 = np.where(bad[:, None], c2[rng.permutation(n)] + rng.normal(0, 1.0, (n, 3)), c2)
    c2[bad, 2] = np.maximum(c2[bad, 2], 0.5)

    def octave(c):
        return np.clip(np.round(np.log(20.0 / c[:, 2]) / np.log(1.2)), 0, n_levels - 1).astype(np.int64)

    def noisy(c, octv, unit):
        """unit: metres per map unit (keyframe 2's map is the true scale smaller)"""
        if not noise:
            return c
        z = c[:, 2:3]
        lateral = rng.normal(0, 0.7, (n, 2)) * (1.2 ** octv)[:, None] * z / cam["fx"]
        along = rng.normal(0, 0.5, (n, 1)) * z * z * unit / (cam["mb"] * cam["fx"])
        d = c / np.linalg.norm(c, axis=1, keepdims=True)
        return c + np.concatenate([lateral, np.zeros((n, 1))], 1) + along * d

    o1, o2 = octave(c1), octave(c2 * s12)
    c1n, c2n = noisy(c1, o1, 1.0), noisy(c2, o2, s12)
    pairs = np.zeros(n, PAIR_DTYPE)
    pairs["Xw1"], pairs["Xw2"] = (c1n - t1) @ R1, (c2n - t2) @ R2
    pairs["max_err1"], pairs["max_err2"] = bounds(o1, n_levels), bounds(o2, n_levels)
    triples = np.stack([rng.permutation(n)[:3] for _ in range(H)]).astype(np.int32) if H else np.zeros((0, 3), np.int32)
    good = np.nonzero(~bad)[0]
    for h in plant:
        triples[h] = rng.permutation(good)[:3]
    return dict(view1=make_view(R1, t1), view2=make_view(R2, t2), pairs=pairs, triples=triples, fix_scale=bool(fix_scale),
                min_inliers=MIN_INLIERS, truth=(s12, R12, t12), bad=bad, oct1=o1, oct2=o2, n_levels=n_levels)


def case_scene(name, **over):
    return make_scene(**{**CASES[name], **over})


def run(scene, mode):
    return solve(scene["view1"], scene["view2"], scene["pairs"], scene["triples"], scene["fix_scale"], mode)


def transform_errors(s, R, t, ref):
    """(e_s, e_R, e_t) of (H) records against the reading `ref`: relative, Frobenius, relative to |t|"""
    rs, rR, rt = ref["s"].astype(F64), ref["R"].astype(F64), ref["t"].astype(F64)
    e_s = np.abs(np.asarray(s, F64) - rs) / np.abs(rs)
    e_R = np.sqrt(((np.asarray(R, F64).reshape(-1, 3, 3) - rR) ** 2).sum((1, 2)))
    e_t = np.linalg.norm(np.asarray(t, F64) - rt, axis=1) / np.linalg.norm(rt, axis=1)
    return e_s, e_R, e_t


def words_to_bits(words, n):
    w = np.ascontiguousarray(words, np.uint64)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")[..., :n].astype(bool)


# ---- the criteria an implementation is held to, shared by the CPU suite (host build of the arithmetic) and the GPU suite -------------
def check_against_yardstick(name, scene, r64, r32, hyps, words, result=None):
    """hyps: orbfe_sim3_hypothesis records (H), words: uint64 (H, ceil(n / 64)), result: an orbfe_sim3_result or None.  Prints every
    figure before it asserts; returns the ratios of the error criterion."""
    n, H, min_inliers = len(scene["pairs"]), len(scene["triples"]), scene["min_inliers"]
    par, par_h = r64["parity"], r64["parity_h"]
    bits = words_to_bits(words, n)
    loose = (~par).sum(1)
    assert np.array_equal(bits[par], r32["inl"][par]), f"{name}: inlier bits differ from R32 on parity decisions"
    got = hyps["n_inliers"].astype(np.int64)
    assert np.array_equal(got, bits.sum(1)), "the count is the popcount of the word row"
    lo = (r32["inl"] & par).sum(1)
    assert ((got >= lo) & (got <= lo + loose)).all(), f"{name}: counts leave the room the non-parity decisions give"
    if result is not None:
        # the select kernel, exactly: the rule over the DEVICE's counts
        want_ret, want_best = select(got, min_inliers)
        assert (int(result["returned"]), int(result["best"])) == (want_ret, want_best)
        assert int(result["best_inliers"]) == (got[want_best] if want_best >= 0 else 0)
        assert int(result["n_inliers"]) == (got[want_ret] if want_ret >= 0 else 0)
        # against the reading, wherever no borderline decision at or before its choice could change a comparison
        hi = lo + loose
        r_ret, r_best = select(r32["count"], min_inliers)
        if r_ret >= 0:
            comparable = (hi[:r_ret] <= min_inliers).all() and lo[r_ret] > min_inliers
        else:
            comparable = (hi <= min_inliers).all() and (lo[r_best] >= hi[:r_best]).all() and (lo[r_best] > hi[r_best + 1:]).all()
        print(f"{name}: returned {want_ret} best {want_best} ({got[want_best] if want_best >= 0 else 0} inliers); reading {r_ret} "
              f"{r_best}; comparable {bool(comparable)}")
        if comparable:
            assert (want_ret, want_best) == (r_ret, r_best)
    # errors of s, R, t against the truth, next to the float reading's own (profiles/create_new_map_points.md: the 4x + 2 ulp rule)
    ulp, ratios = 2.0 ** -23, {}
    if scene["fix_scale"]:
        assert (hyps["s"][par_h] == np.float32(1.0)).all()
    for label, eg, e32 in zip(("s", "R", "t"), transform_errors(hyps["s"][par_h], hyps["R"][par_h], hyps["t"][par_h],
                                                               {k: r64[k][par_h] for k in ("s", "R", "t")}),
                              transform_errors(r32["s"][par_h], r32["R"][par_h], r32["t"][par_h],
                                               {k: r64[k][par_h] for k in ("s", "R", "t")})):
        med = (np.median(eg), np.median(e32))
        mx = (eg.max(), e32.max())
        ratios[label] = (med[0] / med[1] if med[1] > 0 else 0.0, mx[0] / mx[1] if mx[1] > 0 else 0.0)
        print(f"{name}: {par_h.sum()} parity hypotheses, {label}: e(R32) median {med[1]:.3g} max {mx[1]:.3g}; e(got) median {med[0]:.3g} "
              f"max {mx[0]:.3g}; ratios {ratios[label][0]:.3f} {ratios[label][1]:.3f}")
        assert med[0] <= 4 * med[1] + 2 * ulp and mx[0] <= 4 * mx[1] + 2 * ulp, (name, label)
    return ratios
