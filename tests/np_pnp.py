"""A numpy reading of PnPsolver (L/src/PnPsolver.cc, L/ = Source/Libraries/ORB_SLAM2/): SetRansacParameters (:119-156), the sampling
of iterate (:184-197), compute_pose (:451-500) with everything below it, CheckInliers (:291-320), Refine (:248-289) and the
acceptance rule of iterate (:205-243).  The yardstick of tests/test_pnp_cpu.py, tests/test_pnp_gpu.py and
tests/test_pnp_dropin_cpp.py.  Written from the reference's source, not from csrc/pnp_internal.h, and structured differently on
purpose: every step is an array over (solve, ...), the correspondences of a solve are a padded row with a 0 / 1 weight, and the
linear algebra is LAPACK's (eigh, svd, lstsq, qr).

What "equal to the reference" means here.  With four points the EPnP matrix M is 8 x 12 and MtM has a four-dimensional null space:
the four vectors cvSVD returns for it are an arbitrary basis, and the rest of EPnP (find_betas_approx_{1,2,3} each drop different
quadratic terms) depends on that basis.  Each PCA axis of the control points has a free sign as well.  So the implementation under
test exports its CONVENTIONS per solve -- the control points cws and the four vectors V -- and reading() continues from them: it
computes its own centroid and PCA and takes only the SIGN of each axis from cws, and it uses V as given.  Before that,
check_conventions() holds the conventions against LAPACK: the centroid and the axes equal eigh's up to sign, V is orthonormal, for
a minimal solve span(V) equals the span of eigh's four smallest eigenvectors (largest principal angle) and |MtM v| is small against
the largest eigenvalue, for a refine solve (n >= 10) each vector equals eigh's up to sign.  The bounds of those checks are not
constants: per case, the same quantity is measured between two independent float64 solvers of the reading itself -- eigh of MtM
against the right singular vectors of M, eigh of the 3 x 3 against the svd of the centred points -- and ten times the largest value
is allowed, because the implementation forms MtM as eigh's input does and errs in the same way.  The second solver starts at the
PCA (svd of the centred points, LU inverse), so that what the small PCA eigenvalue of a nearly coplanar set does to M is part of the
measured disagreement.  An axis is read back from two exported control points sqrt(d / n) apart, which costs 4 eps |cws| / that
distance of its direction; that representation error is taken off before the comparison.  Measured on the committed cases
(largest per case, test_pnp_cpu.py prints them with -s; the host build and the device give the same figures):
  quantity                      reading's two solvers     implementation     bound (10 x, floor CONV_FLOOR = 64 eps)
  axes                          6e-16 .. 1e-14            below the read-back allowance
  orthonormality of V           1e-15 .. 2e-15            2.4e-15 .. 4.7e-15  1.4e-14 .. 2e-14
  minimal solve: span angle     7e-15 .. 1.1e-8           8e-15 .. 1.5e-8     7e-14 .. 1.1e-7   (grows with lambda_max / lambda_5)
  minimal solve: |MtM v| / max  8e-16 .. 5.9e-10          1.1e-15 .. 7.8e-10  1.4e-14 .. 5.9e-9
  refine solve: vectors         1.3e-15 .. 1e-14          1.8e-15 .. 3.3e-14  1.4e-14 .. 1e-13
CONV_FLOOR is the size of an orthonormality defect that a product of a hundred plane rotations in double cannot avoid (each
contributes eps / 2).

Margin verdicts.  A solve is a PARITY solve when its pose moves by at most POSE_TOL (on R and on t / max(1, |t|)) on repeating the
reading with V perturbed by seeded noise of size BASIS_NOISE, and when the gaps that adopting a sign needs are there: the PCA
eigenvalues separated by EIG_GAP of the largest, and for a refine solve the five smallest eigenvalues of MtM separated by EIG_GAP of
the fifth.  A solve whose reading is not finite (a coplanar or repeated set: 0 / 0 in the inverse of the control-point matrix) is a
DEGENERATE solve: every comparison of CheckInliers is false, and the verdicts -- all false -- are parity decisions.  A (solve,
correspondence) decision is a PARITY decision when the solve is one and error2 is at least ERR_MARGIN x bound away from the bound.
Re-measured with this reading on the committed cases: noise of BASIS_NOISE = 1e-10 on V moves the pose of a parity solve by at
most 1.2e-7 (a factor of about a thousand, one order below POSE_TOL = 1e-6); the implementation's poses differ from the reading's by
at most 4.7e-12 on minimal and 1.6e-14 on refine solves.  No solve of any case is outside the margins (the two planted singular sets
are DEGENERATE, not non-parity) and at most 1 decision in 2000 is (test_pnp_cpu.py::test_non_parity_cap_under_the_reading_alone).
Which start won is compared where the two smallest reprojection errors are further apart than ten times what that noise moves
them: three starts that converge to one pose tie to rounding, and the tie decides nothing."""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
EIG_GAP, ERR_MARGIN, NON_PARITY_CAP = 1e-3, 1e-2, 0.03      # np_sim3.py's values
BASIS_NOISE, POSE_TOL = 1e-10, 1e-6
CONV_FLOOR = 64 * 2.0 ** -52
CALL_SITE = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)   # Tracking.cc:1262

POINT_DTYPE = np.dtype([("Xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("max_err", "<f4")])
KITTI = dict(fx=718.856, fy=718.856, cx=607.19, cy=185.2, width=1241, height=376)


# ---- SetRansacParameters, the draws, the rule of iterate ---------------------------------------------------------------------------
def ransac_parameters(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """:119-151, literally: (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)"""
    eps = F32(epsilon)
    n_min = int(F32(N) * eps)                     # int = int * float
    n_min = max(n_min, min_inliers, min_set)
    if eps < F32(n_min) / F32(N):
        eps = F32(n_min) / F32(N)
    if n_min == N:
        its = 1
    else:
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(1 - F64(probability)) / np.log(1 - F64(eps) ** 3))
        its = 1 if not v >= 1 else (max_iterations if v >= max_iterations else int(v))
    return n_min, max(1, min(its, max_iterations)), eps


def draw_sets_literal(n, H, below):
    """:184-197 with a list, as written"""
    out = []
    for _ in range(H):
        avail = list(range(n))
        row = []
        for _ in range(4):
            randi = below(len(avail))
            row.append(avail[randi])
            avail[randi] = avail[-1]
            avail.pop()
        out.append(row)
    return np.asarray(out, np.int32).reshape(H, 4)


def find_rule(counts, refine_counts, min_inliers):
    """find() = iterate(mRansacMaxIts) over the evaluated hypotheses (:179-243): (returned, refined, best, best_count).
    refine_counts[h] is read only where h is the best so far."""
    best, best_count = -1, 0
    for h, c in enumerate(counts):
        if c >= min_inliers:
            if c > best_count:
                best, best_count = h, int(c)
            if refine_counts[best] > min_inliers:
                return h, True, best, best_count
    if best_count >= min_inliers:
        return best, False, best, best_count
    return -1, False, -1, 0


def prefix_maxima(counts, min_inliers):
    """the hypotheses that become mvbBestInliers (:207): count >= min_inliers and strictly above every earlier count"""
    out, top = [], 0
    for h, c in enumerate(counts):
        if c >= min_inliers and c > top:
            out.append(h)
        top = max(top, int(c))
    return out


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def _rodrigues(rv):
    a = np.linalg.norm(rv)
    k = np.asarray(rv, F64) / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def _project(cam, R, t, X):
    c = X.astype(F64) @ R.T + t
    return np.stack([cam["fx"] * c[:, 0] / c[:, 2] + cam["cx"], cam["fy"] * c[:, 1] / c[:, 2] + cam["cy"]], -1)


def _scene_points(rng, cam, R, t, n, noise, th2):
    """n correspondences of the pose (R, t): float32 world points in front of the camera, keypoints with octave-scaled noise"""
    uv = np.stack([rng.uniform(20, cam["width"] - 20, n), rng.uniform(20, cam["height"] - 20, n)], -1)
    z = rng.uniform(5.0, 30.0, n)
    c = np.stack([(uv[:, 0] - cam["cx"]) / cam["fx"] * z, (uv[:, 1] - cam["cy"]) / cam["fy"] * z, z], -1)
    Xw = ((c - t) @ R).astype(F32)
    octave = rng.integers(0, 8, n)
    sigma2 = (F32(1.2) ** octave.astype(F32)) ** 2
    p = np.zeros(n, POINT_DTYPE)
    p["Xw"] = Xw
    kp = _project(cam, R, t, Xw) + rng.normal(0, 1, (n, 2)) * noise * np.sqrt(sigma2.astype(F64))[:, None]
    p["u"], p["v"] = kp[:, 0].astype(F32), kp[:, 1].astype(F32)
    p["max_err"] = sigma2.astype(F32) * F32(th2)
    return p


def _outliers(rng, cam, p, idx):
    p["u"][idx] = rng.uniform(0, cam["width"], len(idx)).astype(F32)
    p["v"][idx] = rng.uniform(0, cam["height"], len(idx)).astype(F32)


def make_scene(n_in, n_out, noise, seed, cam=KITTI):
    """n_in correspondences of one seeded pose followed by n_out gross outliers: dict(cam, points, truth)"""
    rng = np.random.default_rng([seed, n_in, n_out])
    cam = dict(cam, **{k: float(F32(cam[k])) for k in ("fx", "fy", "cx", "cy")})
    R = _rodrigues(rng.normal(0, 0.15, 3)).astype(F32).astype(F64)
    t = rng.normal(0, 1.0, 3).astype(F32).astype(F64)
    p = _scene_points(rng, cam, R, t, n_in + n_out, noise, CALL_SITE["th2"])
    _outliers(rng, cam, p, np.arange(n_in, n_in + n_out))
    return dict(cam=cam, points=p, truth=(R, t))


CASES = ("kitti", "single_iteration", "too_few", "best_at_exhaustion", "second_best_refines", "degenerate_sets")


def make_case(name, seed=7, cam=KITTI):
    """A seeded case: dict(cam, points, sets, params, min_inliers, iterations, truth=(R, t), planted).  Camera, pose and world points
    are float32 values.  The sets are the draws of :184-197 from the seeded generator, with the planted ones put in place."""
    rng = np.random.default_rng([seed, CASES.index(name)])
    cam = dict(cam, **{k: float(F32(cam[k])) for k in ("fx", "fy", "cx", "cy")})
    R = _rodrigues(rng.normal(0, 0.15, 3)).astype(F32).astype(F64)
    t = rng.normal(0, 1.0, 3).astype(F32).astype(F64)
    params = dict(CALL_SITE)
    planted = {}
    below = lambda k: int(rng.integers(k))
    if name == "kitti":                       # a relocalisation candidate: 60 matches, 0.7 px, 30 % gross outliers -> 35 hypotheses
        p = _scene_points(rng, cam, R, t, 60, 0.7, params["th2"])
        _outliers(rng, cam, p, rng.permutation(60)[:18])
    elif name == "single_iteration":          # nMinInliers == N: one iteration (:146)
        p = _scene_points(rng, cam, R, t, 10, 0.3, params["th2"])
    elif name == "too_few":                   # N < nMinInliers: nothing is evaluated (:171)
        p = _scene_points(rng, cam, R, t, 8, 0.3, params["th2"])
    elif name == "best_at_exhaustion":        # ten exact inliers of twenty: a count of 10 qualifies (>=), its refine never exceeds 10
        p = _scene_points(rng, cam, R, t, 20, 0.02, params["th2"])
        _outliers(rng, cam, p, np.arange(10, 20))
        planted = {2: [0, 3, 6, 9], 11: [1, 4, 5, 8]}
    elif name == "second_best_refines":       # twenty points of another pose first (refine == 20, fails), then 28 of the true one
        params.update(epsilon=0.4)
        p = _scene_points(rng, cam, R, t, 50, 0.3, params["th2"])
        R2, t2 = _rodrigues(np.array([0.3, -0.4, 0.2])), t + np.array([2.0, -1.0, 3.0])
        q = _scene_points(rng, cam, R2, t2, 20, 0.02, params["th2"])
        p[28:48] = q
        _outliers(rng, cam, p, np.arange(48, 50))
        planted = {0: [28, 33, 39, 46], 3: [1, 9, 17, 25]}
    elif name == "degenerate_sets":           # kitti with a coplanar set and a set with a repeated point, both exactly singular
        p = _scene_points(rng, cam, R, t, 60, 0.7, params["th2"])
        _outliers(rng, cam, p, 8 + rng.permutation(52)[:18])
        p["Xw"][0:4, 2] = F32(8.0)            # four points of the plane z = 8: the centred z column is exactly zero
        p["Xw"][4:8, 2] = F32(9.0)
        p[5] = p[4]                           # the same map point and keypoint twice
        planted = {5: [0, 1, 2, 3], 9: [4, 5, 6, 7]}
    else:
        raise KeyError(name)
    n = len(p)
    n_min, its, _ = ransac_parameters(n, params["probability"], params["min_inliers"], params["max_iterations"], params["min_set"],
                                      params["epsilon"])
    sets = draw_sets_literal(n, its, below) if n >= 4 else np.zeros((0, 4), np.int32)
    for h, s in planted.items():
        sets[h] = s
    return dict(name=name, cam=cam, points=p, sets=sets, params=params, min_inliers=n_min, iterations=its, truth=(R, t), planted=planted)


# ---- the reading --------------------------------------------------------------------------------------------------------------
def _pad(sel_lists):
    S, mm = len(sel_lists), max([len(s) for s in sel_lists] + [1])
    sel, msk = np.zeros((S, mm), np.int64), np.zeros((S, mm), F64)
    for i, s in enumerate(sel_lists):
        sel[i, :len(s)], msk[i, :len(s)] = s, 1.0
    return sel, msk


def _pca(pw, msk, m):
    c0 = (pw * msk[..., None]).sum(1) / m[:, None]
    pw0 = (pw - c0[:, None]) * msk[..., None]
    cov = np.einsum("sia,sib->sab", pw0, pw0)
    d, ax = np.linalg.eigh(cov)
    return c0, pw0, d[:, ::-1], np.swapaxes(ax, 1, 2)[:, ::-1]          # dc descending, axes as rows


def _epnp_matrix(cam, alphas, uv, msk):
    S, mm = msk.shape
    M = np.zeros((S, mm, 2, 12), F64)
    for i in range(4):
        M[:, :, 0, 3 * i] = alphas[:, :, i] * cam["fx"]
        M[:, :, 0, 3 * i + 2] = alphas[:, :, i] * (cam["cx"] - uv[:, :, 0])
        M[:, :, 1, 3 * i + 1] = alphas[:, :, i] * cam["fy"]
        M[:, :, 1, 3 * i + 2] = alphas[:, :, i] * (cam["cy"] - uv[:, :, 1])
    return (M * msk[:, :, None, None]).reshape(S, 2 * mm, 12)


def _controls(cam, c0, dc, axes, m, pw, uv, msk, lu=False):
    """control points (:382-386), barycentric coordinates (:389-410) and M (:412-426, :457-458)"""
    cws = np.concatenate([c0[:, None], c0[:, None] + np.sqrt(dc / m[:, None])[..., None] * axes], 1)
    CC = np.swapaxes(cws[:, 1:] - cws[:, :1], 1, 2)                 # columns = control point offsets (:394-396)
    okc = np.isfinite(CC).all((1, 2))
    if lu:
        okc &= np.abs(np.linalg.det(np.where(okc[:, None, None], CC, np.eye(3)))) > 0
        CCinv = np.linalg.inv(np.where(okc[:, None, None], CC, np.eye(3)))
    else:
        U, sv, Vt = np.linalg.svd(np.where(okc[:, None, None], CC, np.eye(3)))
        CCinv = np.einsum("sji,sj,skj->sik", Vt, 1.0 / sv, U)       # no threshold: a zero singular value is 0 / 0
    CCinv[~okc] = np.nan
    a123 = np.einsum("sjk,smk->smj", CCinv, pw - c0[:, None])
    alphas = np.concatenate([(1.0 - a123[..., 0] - a123[..., 1] - a123[..., 2])[..., None], a123], -1)
    return cws, alphas, _epnp_matrix(cam, alphas, uv, msk)


_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _lstsq(A, b):
    out = np.full(A.shape[:1] + A.shape[2:], np.nan)
    for s in range(len(A)):
        if np.isfinite(A[s]).all() and np.isfinite(b[s]).all():
            out[s] = np.linalg.lstsq(A[s], b[s], rcond=None)[0]
    return out


def _pose_from_betas(cam, betas, V, alphas, pw, uv, msk, m):
    """compute_R_and_t (:617-627) for one start: R (S,3,3), t (S,3), mean reprojection error (S)"""
    ccs = np.einsum("si,sie->se", betas, V).reshape(-1, 4, 3)
    pcs = np.einsum("smi,sik->smk", alphas, ccs)
    flip = np.where(pcs[:, 0, 2] < 0.0, -1.0, 1.0)                  # solve_for_sign looks at the first point only
    pcs = pcs * flip[:, None, None]
    w = msk[..., None]
    pc0, pw0 = (pcs * w).sum(1) / m[:, None], (pw * w).sum(1) / m[:, None]
    abt = np.einsum("smj,smk->sjk", (pcs - pc0[:, None]) * w, (pw - pw0[:, None]) * w)
    ok = np.isfinite(abt).all((1, 2))
    U, _, Vt = np.linalg.svd(np.where(ok[:, None, None], abt, np.eye(3)))
    R = U @ Vt
    R[np.linalg.det(R) < 0, 2, :] *= -1.0                          # row 2, as written (:586-590)
    R[~ok] = np.nan
    t = pc0 - np.einsum("sjk,sk->sj", R, pw0)
    c = np.einsum("sjk,smk->smj", R, pw) + t[:, None]
    ue, ve = cam["cx"] + cam["fx"] * c[..., 0] / c[..., 2], cam["cy"] + cam["fy"] * c[..., 1] / c[..., 2]
    err = (np.sqrt((uv[..., 0] - ue) ** 2 + (uv[..., 1] - ve) ** 2) * msk).sum(1) / m
    return R, t, err


def check_inliers(cam, R, t, points):
    """CheckInliers (:291-320) of S poses over all n points with the reference's roundings: error2 (S, n) float32 and the verdicts"""
    X = points["Xw"].astype(F64)
    with np.errstate(all="ignore"):
        c = np.einsum("sjk,nk->snj", R, X)
        Xc = (c[..., 0] + t[:, None, 0]).astype(F32)
        Yc = (c[..., 1] + t[:, None, 1]).astype(F32)
        invZc = (1.0 / (c[..., 2] + t[:, None, 2])).astype(F32)
        ue = cam["cx"] + cam["fx"] * Xc.astype(F64) * invZc.astype(F64)
        ve = cam["cy"] + cam["fy"] * Yc.astype(F64) * invZc.astype(F64)
        dx = (points["u"].astype(F64)[None] - ue).astype(F32)
        dy = (points["v"].astype(F64)[None] - ve).astype(F32)
        e2 = dx * dx + dy * dy
        return e2, e2 < points["max_err"][None]


def reading(cam, points, sel_lists, conventions, V_noise=None):
    """compute_pose for S solves in float64.  sel_lists: per solve the indices of its correspondences, in order.  conventions: dict
    with cws (S, 4, 3) and V (S, 4, 12) of the implementation under test; only the sign of each PCA axis is taken from cws, V is used
    as given (plus V_noise).  Returns a dict: R, t, winner, betas (S,3,4), rep_errors (S,3), cws, c0, dc, axes, MtM, M, alphas, finite."""
    sel, msk = _pad(sel_lists)
    m = msk.sum(1)
    cws_in = np.asarray(conventions["cws"], F64).reshape(-1, 4, 3)
    V = np.asarray(conventions["V"], F64).reshape(-1, 4, 12)
    if V_noise is not None:
        V = V + V_noise
    with np.errstate(all="ignore"):
        pw = points["Xw"].astype(F64)[sel]
        uv = np.stack([points["u"], points["v"]], -1).astype(F64)[sel]
        c0, _, dc, axes = _pca(pw, msk, m)
        sign = np.where(np.einsum("ska,ska->sk", axes, cws_in[:, 1:] - cws_in[:, :1]) < 0, -1.0, 1.0)
        axes = axes * sign[..., None]
        cws, alphas, M = _controls(cam, c0, dc, axes, m, pw, uv, msk)
        # the same quantities from the other float64 solvers: the PCA from the svd of the centred points, the inverse from LU
        _, sv0, vt0 = np.linalg.svd((pw - c0[:, None]) * msk[..., None])
        flip0 = np.where(np.einsum("ska,ska->sk", vt0, axes) < 0, -1.0, 1.0)
        M_alt = _controls(cam, c0, sv0 ** 2, vt0 * flip0[..., None], m, pw, uv, msk, lu=True)[2]
        MtM = np.einsum("sra,srb->sab", M, M)
        dv = np.stack([V[:, :, 3 * a:3 * a + 3] - V[:, :, 3 * b:3 * b + 3] for a, b in _PAIRS], 2)      # (S, vector, row, 3)
        dot = lambda x, y: (dv[:, x] * dv[:, y]).sum(-1)
        L = np.stack([dot(0, 0), 2 * dot(0, 1), dot(1, 1), 2 * dot(0, 2), 2 * dot(1, 2), dot(2, 2), 2 * dot(0, 3), 2 * dot(1, 3),
                      2 * dot(2, 3), dot(3, 3)], -1)                                                     # (S, 6, 10)
        rho = np.stack([((cws[:, a] - cws[:, b]) ** 2).sum(-1) for a, b in _PAIRS], -1)
        S = len(sel)
        betas = np.zeros((S, 3, 4))
        b4 = _lstsq(L[:, :, [0, 1, 3, 6]], rho)                          # :632-658
        sg = np.where(b4[:, 0] < 0, -1.0, 1.0)
        betas[:, 0, 0] = np.sqrt(sg * b4[:, 0])
        betas[:, 0, 1:] = sg[:, None] * b4[:, 1:] / betas[:, 0, :1]
        for k, cols in ((1, [0, 1, 2]), (2, [0, 1, 2, 3, 4])):           # :663-722
            b = _lstsq(L[:, :, cols], rho)
            neg = b[:, 0] < 0
            betas[:, k, 0] = np.sqrt(np.where(neg, -b[:, 0], b[:, 0]))
            betas[:, k, 1] = np.where(neg, np.where(b[:, 2] < 0, np.sqrt(-b[:, 2]), 0.0), np.where(b[:, 2] > 0, np.sqrt(b[:, 2]), 0.0))
            betas[:, k, 0] = np.where(b[:, 1] < 0, -betas[:, k, 0], betas[:, k, 0])
            if k == 2:
                betas[:, k, 2] = b[:, 3] / betas[:, k, 0]
        for k in range(3):                                                # gauss_newton (:774-816): five least-squares steps
            for _ in range(5):
                b0, b1, b2, b3 = (betas[:, k, i][:, None] for i in range(4))
                A = np.stack([2 * L[..., 0] * b0 + L[..., 1] * b1 + L[..., 3] * b2 + L[..., 6] * b3,
                              L[..., 1] * b0 + 2 * L[..., 2] * b1 + L[..., 4] * b2 + L[..., 7] * b3,
                              L[..., 3] * b0 + L[..., 4] * b1 + 2 * L[..., 5] * b2 + L[..., 8] * b3,
                              L[..., 6] * b0 + L[..., 7] * b1 + L[..., 8] * b2 + 2 * L[..., 9] * b3], -1)
                r = rho - (L[..., 0] * b0 * b0 + L[..., 1] * b0 * b1 + L[..., 2] * b1 * b1 + L[..., 3] * b0 * b2 + L[..., 4] * b1 * b2 +
                           L[..., 5] * b2 * b2 + L[..., 6] * b0 * b3 + L[..., 7] * b1 * b3 + L[..., 8] * b2 * b3 + L[..., 9] * b3 * b3)
                fin = np.isfinite(A).all((1, 2)) & np.isfinite(r).all(1)
                x = np.einsum("sji,si->sj", np.linalg.pinv(np.where(fin[:, None, None], A, 0.0)), r)   # qr_solve: the least-squares step
                x[~fin] = np.nan
                betas[:, k] += x
        Rs, ts, errs = zip(*[_pose_from_betas(cam, betas[:, k], V, alphas, pw, uv, msk, m) for k in range(3)])
        errs = np.stack(errs, -1)
        winner = np.zeros(S, np.int64)
        winner[errs[:, 1] < errs[:, 0]] = 1
        winner[errs[:, 2] < errs[np.arange(S), winner]] = 2
        R = np.stack(Rs, 1)[np.arange(S), winner]
        t = np.stack(ts, 1)[np.arange(S), winner]
        finite = np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1)
    return dict(R=R, t=t, winner=winner, betas=betas, rep_errors=errs, cws=cws, c0=c0, dc=dc, axes=axes, M=M, M_alt=M_alt, MtM=MtM, alphas=alphas,
                finite=finite, m=m)


# ---- the conventions against LAPACK ---------------------------------------------------------------------------------------------
def _angle(A, B):
    """sine of the largest principal angle between the row spaces of two orthonormal (k, 12) sets"""
    return float(np.linalg.svd(A - (A @ B.T) @ B, compute_uv=False)[0])          # what of A lies outside span(B)


def _vec_diff(a, b):
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


def convention_measures(rd, conventions, sel_lists, points):
    """Per solve, the quantities of check_conventions for the implementation (key 'impl') and for the reading's two own solvers
    against each other (key 'self'); NaN where a solve is not finite.  Keys of each: centroid, axes, orth, span, resid, vectors."""
    S = len(sel_lists)
    cws_in = np.asarray(conventions["cws"], F64).reshape(-1, 4, 3)
    V = np.asarray(conventions["V"], F64).reshape(-1, 4, 12)
    out = {k: {q: np.full(S, np.nan) for q in ("centroid", "axes", "orth", "span", "resid", "vectors")} for k in ("impl", "self")}
    for s in range(S):
        if not rd["finite"][s] or not np.isfinite(V[s]).all() or not np.isfinite(cws_in[s]).all():
            continue
        m = int(rd["m"][s])
        scale = max(1.0, np.abs(rd["c0"][s]).max())
        out["impl"]["centroid"][s] = np.abs(cws_in[s, 0] - rd["c0"][s]).max() / scale
        pw0 = points["Xw"].astype(F64)[sel_lists[s]] - rd["c0"][s]
        d = cws_in[s, 1:] - cws_in[s, :1]
        # an axis is read back from two control points k = sqrt(d / n) apart: that difference carries the rounding of the
        # coordinates themselves, 4 eps |cws| / k of the direction, which is not the implementation's error and is taken off
        lost = [4 * 2.0 ** -52 * max(1.0, np.abs(cws_in[s]).max()) / np.linalg.norm(d[i]) for i in range(3)]
        out["impl"]["axes"][s] = max(max(0.0, np.abs(d[i] / np.linalg.norm(d[i]) - rd["axes"][s, i]).max() - lost[i]) for i in range(3))
        _, _, vt = np.linalg.svd(pw0)                                         # the other solver of the same axes
        out["self"]["axes"][s] = max(_vec_diff(vt[i], rd["axes"][s, i]) for i in range(3))
        out["self"]["centroid"][s] = np.abs(pw0.sum(0)).max() / m / scale
        lam, E = np.linalg.eigh(rd["MtM"][s])
        E4 = E[:, :4].T
        W4 = np.linalg.svd(rd["M_alt"][s][:2 * m], full_matrices=True)[2][::-1][:4]
        out["impl"]["orth"][s] = np.abs(V[s] @ V[s].T - np.eye(4)).max()
        out["self"]["orth"][s] = max(np.abs(E4 @ E4.T - np.eye(4)).max(), np.abs(W4 @ W4.T - np.eye(4)).max())
        if m < 6:                                                             # a null space: the span, and the residual
            out["impl"]["span"][s], out["self"]["span"][s] = _angle(V[s], E4), _angle(W4, E4)
            out["impl"]["resid"][s] = np.abs(rd["MtM"][s] @ V[s].T).max() / lam[-1]
            out["self"]["resid"][s] = max(np.abs(rd["MtM"][s] @ E4.T).max(), np.abs(rd["MtM"][s] @ W4.T).max()) / lam[-1]
        else:
            out["impl"]["vectors"][s] = max(_vec_diff(V[s, i], E4[i]) for i in range(4))
            out["self"]["vectors"][s] = max(_vec_diff(W4[i], E4[i]) for i in range(4))
    return out


def check_conventions(measures, use):
    """Every quantity of the implementation on the solves `use` (bool) is at most ten times the largest disagreement of the
    reading's own two solvers on them (CONV_FLOOR at least).  Returns the table {quantity: (largest of impl, largest of self,
    bound)}; raises AssertionError with it."""
    table = {}
    for q in measures["impl"]:
        a, b = measures["impl"][q][use], measures["self"][q][use]
        a, b = a[np.isfinite(a)], b[np.isfinite(b)]
        if len(a) == 0:
            continue
        ref = float(b.max()) if len(b) else 0.0
        table[q] = (float(a.max()), ref, max(10.0 * ref, CONV_FLOOR))
    bad = {q: v for q, v in table.items() if not v[0] <= v[2]}
    assert not bad, f"conventions outside ten times the reading's own disagreement: {bad}"
    return table


def lapack_conventions(cam, points, sel_lists):
    """Conventions from LAPACK alone -- eigh's axes with their signs, eigh's four smallest eigenvectors of the reading's own MtM --
    for judging the scenes without any implementation."""
    S = len(sel_lists)
    sel, msk = _pad(sel_lists)
    m = msk.sum(1)
    c0, _, dc, axes = _pca(points["Xw"].astype(F64)[sel], msk, m)
    with np.errstate(all="ignore"):
        cws = np.concatenate([c0[:, None], c0[:, None] + np.sqrt(dc / m[:, None])[..., None] * axes], 1)
    rd = reading(cam, points, sel_lists, dict(cws=cws, V=np.zeros((S, 4, 12))))
    V = np.zeros((S, 4, 12))
    for s in range(S):
        if np.isfinite(rd["MtM"][s]).all():
            V[s] = np.linalg.eigh(rd["MtM"][s])[1][:, :4].T
    return dict(cws=cws, V=V)


# ---- margin verdicts ------------------------------------------------------------------------------------------------------------
def _pose_move(a, b):
    dR = np.abs(a["R"] - b["R"]).max((1, 2))
    tn = np.maximum(1.0, np.linalg.norm(a["t"], axis=1))
    return np.maximum(dR, np.abs(a["t"] - b["t"]).max(1) / tn)


def verdicts(cam, points, sel_lists, conventions, seed=11):
    """The reading and its margin verdicts.  Adds to reading()'s dict: degenerate (S), parity (S), move (S), error2 (S, n), inl (S, n),
    count (S), decisions (S, n) bool = the PARITY decisions."""
    rd = reading(cam, points, sel_lists, conventions)
    rng = np.random.default_rng(seed)
    noisy = reading(cam, points, sel_lists, conventions, rng.normal(0, BASIS_NOISE, (len(sel_lists), 4, 12)))
    with np.errstate(all="ignore"):
        move = _pose_move(rd, noisy)
        dc = rd["dc"]
        gaps = ((dc[:, 0] - dc[:, 1]) >= EIG_GAP * dc[:, 0]) & ((dc[:, 1] - dc[:, 2]) >= EIG_GAP * dc[:, 0])
        lam = np.linalg.eigvalsh(np.where(np.isfinite(rd["MtM"]), rd["MtM"], 0.0))[:, :5]
        refine = rd["m"] >= 6
        gaps &= ~refine | (np.diff(lam, axis=1) >= EIG_GAP * lam[:, 4:5]).all(1)
        degenerate = ~rd["finite"]
        parity = rd["finite"] & noisy["finite"] & (move <= POSE_TOL) & gaps
        # which start won can be compared where the two smallest errors are further apart than ten times what the noise moves them
        es = np.sort(rd["rep_errors"], 1)
        winner_parity = parity & (rd["winner"] == noisy["winner"]) & \
            ((es[:, 1] - es[:, 0]) >= 10.0 * np.abs(rd["rep_errors"] - noisy["rep_errors"]).max(1))
        e2, inl = check_inliers(cam, rd["R"], rd["t"], points)
        bound = points["max_err"][None].astype(F64)
        decisions = (parity[:, None] & (np.abs(e2.astype(F64) - bound) >= ERR_MARGIN * bound)) | degenerate[:, None]
    rd.update(degenerate=degenerate, parity=parity, winner_parity=winner_parity, move=move, error2=e2, inl=inl, count=inl.sum(1), decisions=decisions, lam5=lam)
    return rd


def unpack_bits(words, n):
    w = np.ascontiguousarray(words, np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :n].astype(bool)


def check_against_yardstick(case, sol, report=None):
    """sol: the implementation's records for case['sets'] -- result, mask, hyps, words, refines, refine_words, diag, refine_diag (the
    PnpSolution of refactored_orb_slam2_amd.pnp or the same from the host build).  Asserts everything the module docstring promises
    and returns a dict of the measured figures."""
    cam, pts, sets, n_min = case["cam"], case["points"], case["sets"], case["min_inliers"]
    n, H = len(pts), len(sets)
    res = sol.result
    fig = {}
    if n < n_min or H == 0:
        assert res["returned"] == -1 and res["best"] == -1 and res["n_inliers"] == 0 and not np.asarray(sol.mask).any()
        return fig
    words, rwords = unpack_bits(sol.words, n), unpack_bits(sol.refine_words, n)
    counts = sol.hyps["n_inliers"]
    tail = (-n) % 64
    if tail:
        assert not (np.asarray(sol.words, np.uint64)[:, -1] >> np.uint64(64 - tail)).any(), "tail bits of the last word"
        assert not (np.asarray(sol.refine_words, np.uint64)[:, -1] >> np.uint64(64 - tail)).any()
    assert np.array_equal(counts, words.sum(1)), "a count is the popcount of its row"
    # the selection is exactly the rule on the implementation's own counts
    pm = prefix_maxima(counts, n_min)
    assert np.array_equal(np.flatnonzero(sol.hyps["refine"] >= 0), pm) and all(sol.hyps["refine"][h] == h for h in pm), "refine rows"
    rc = sol.refines["n_inliers"]
    assert np.array_equal(rc[pm], rwords[pm].sum(1)) and np.array_equal(sol.refines["success"][pm] != 0, rc[pm] > n_min)
    ret, refined, best, best_count = find_rule(counts, rc, n_min)
    assert (res["returned"], bool(res["refined"]), res["best"], res["best_inliers"]) == (ret, refined, best, best_count), "selection"
    if best >= 0:
        rec = sol.refines[best] if refined else sol.hyps[best]
        Tcw = np.concatenate([rec["R"].reshape(3, 3), rec["t"].reshape(3, 1)], 1).astype(F32).reshape(12)
        assert np.array_equal(res["Tcw"], Tcw) and res["n_inliers"] == rec["n_inliers"], "Tcw is the rounding of the doubles"
        assert np.array_equal(unpack_bits(sol.mask, n), (rwords if refined else words)[best])
    else:
        assert res["n_inliers"] == 0 and not res["Tcw"].any() and not np.asarray(sol.mask).any()
    # the two families of solves against the reading
    for kind, rows, sel_lists, recs, bits, dg in (
            ("minimal", np.arange(H), [list(map(int, s)) for s in sets], sol.hyps, words, sol.diag),
            ("refine", np.asarray(pm, np.int64), [list(np.flatnonzero(words[h])) for h in pm], sol.refines, rwords, sol.refine_diag)):
        if len(rows) == 0:
            continue
        conv = dict(cws=dg["cws"][rows], V=dg["V"][rows])
        vd = verdicts(cam, pts, sel_lists, conv)
        par = vd["parity"]
        meas = convention_measures(vd, conv, sel_lists, pts)
        fig[kind + "_conventions"] = check_conventions(meas, par)
        R, t = recs["R"][rows].reshape(-1, 3, 3), recs["t"][rows]
        with np.errstate(all="ignore"):
            move = _pose_move(dict(R=R, t=t), vd)
        fig[kind + "_pose"] = float(move[par].max()) if par.any() else 0.0
        assert (move[par] <= POSE_TOL).all(), f"{kind}: poses of parity solves differ from the reading by {move[par].max()}"
        wp = vd["winner_parity"]
        assert np.array_equal(recs["winner"][rows][wp], vd["winner"][wp]), f"{kind}: which start won"
        dec = vd["decisions"]
        assert np.array_equal(bits[rows][dec], vd["inl"][dec]), f"{kind}: inlier bits differ on parity decisions"
        room = (~dec).sum(1)
        diff = np.abs(recs["n_inliers"][rows].astype(np.int64) - (vd["inl"] & dec).sum(1) - ((bits[rows] & ~dec).sum(1)))
        assert (diff == 0).all() and (np.abs(recs["n_inliers"][rows] - vd["count"]) <= room).all(), f"{kind}: counts"
        dgn = vd["degenerate"]
        assert (recs["n_inliers"][rows][dgn] == 0).all() and not bits[rows][dgn].any(), f"{kind}: a degenerate solve has no inliers"
        fig[kind + "_non_parity"] = (int((~par & ~dgn).sum()), len(rows), int((~dec).sum()), dec.size)
        if report is not None:
            report.append((kind, vd, meas))
    return fig
