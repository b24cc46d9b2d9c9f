"""A float64 numpy / plain-Python reading of Optimizer::OptimizeSim3 (L/src/Optimizer.cc:1381-1573) and of the parts of g2o it runs
(G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o): the yardstick of tests/test_optsim3_cpu.py and tests/test_optsim3_gpu.py.  Written
from the reference's sources (G/types/sim3/sim3.h, types_seven_dof_expmap.h, G/core/base_fixed_sized_edge.hpp), not from
csrc/optsim3_internal.h, and structured differently on purpose: a transform is a (quaternion, translation, scale) tuple of Python
floats, the edges are numpy columns -- row 2 k is e12 of correspondence k, row 2 k + 1 its e21, the order of addEdge -- the 15
transforms of a numeric Jacobian are applied to whole columns, and H, b and chi are accumulated SEQUENTIALLY in that row order
(np.cumsum adds left to right).  Eigen's quaternion formulas, the Huber columns and the summer are those of tests/np_pose.py.

The chi2 convention is the documented one of the library (include/orbfe.h): a correspondence is classified by its chi2 at the final
estimate of the optimize() call, where the reference reads what the last Levenberg trial left in the edge.

No Eigen or g2o can be built where this runs, so this is a reading, unpinned.  Known liberties: the 7 x 7
block is solved by an unpivoted LDL^T where BlockSolverX / LinearSolverEigen runs SimplicialLLT; Eigen's fixed-size products are
taken in index order.  Everything is double; inputs are the floats the ABI carries, widened."""
from __future__ import annotations

import math

import numpy as np

from tests import np_pose as P

F32 = np.float32
EPS = 0.00001


# ---- g2o::Sim3 (G/types/sim3/sim3.h): (q = [x, y, z, w], t = [x, y, z], s) ---------------------------------------------------------
def sim3_from_floats(v):
    """Sim3(Matrix3, Vector3, double) (:56-59) of s, R (row-major), t as 13 floats: Quaternion(R), normalizeRotation"""
    v = [float(x) for x in np.asarray(v, F32).reshape(13)]
    R = [v[1:4], v[4:7], v[7:10]]
    return P.quat_normalized(P.quat_from_matrix(R)), v[10:13], v[0]


def sim3_to_floats(S):
    """scale(), rotation().toRotationMatrix(), translation() -> 13 doubles"""
    q, t, s = S
    R = P.quat_to_matrix(q)
    return np.array([s] + R[0] + R[1] + R[2] + list(t), np.float64)


def sim3_exp(u):
    """Sim3(const Vector7&) (:61-124): omega, upsilon, sigma.  The quaternion is NOT normalised here."""
    om = [float(u[0]), float(u[1]), float(u[2])]
    up = [float(u[3]), float(u[4]), float(u[5])]
    sigma = float(u[6])
    theta = math.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    s = math.exp(sigma)
    Om2 = P._mat3_mul(Om, Om)
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]

    def full_R():
        a, b = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
        return [[eye[i][j] + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]

    def small_R():
        return [[eye[i][j] + Om[i][j] + Om2[i][j] / 2 for j in range(3)] for i in range(3)]

    if abs(sigma) < EPS:
        C = 1.0
        if theta < EPS:
            A, B = 1.0 / 2.0, 1.0 / 6.0
            R = small_R()
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
            R = full_R()
    else:
        C = (s - 1) / sigma
        if theta < EPS:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s - 1) / (sigma2 * sigma)
            R = small_R()
        else:
            R = full_R()
            a, b = s * math.sin(theta), s * math.cos(theta)
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1 / theta2
    W = [[A * Om[i][j] + B * Om2[i][j] + C * eye[i][j] for j in range(3)] for i in range(3)]
    t = [W[i][0] * up[0] + W[i][1] * up[1] + W[i][2] * up[2] for i in range(3)]
    return P.quat_from_matrix(R), t, s


def sim3_map(S, v):
    """map (:126): s * (r * xyz) + t; v three scalars or three columns"""
    q, t, s = S
    r = P.quat_rotate(q, v)
    return s * r[0] + t[0], s * r[1] + t[1], s * r[2] + t[2]


def sim3_mul(a, b):
    """operator* (:226-232): no normalisation"""
    return P.quat_mul(a[0], b[0]), list(sim3_map(a, b[1])), a[2] * b[2]


def sim3_inverse(S):
    """inverse (:200-202): Sim3(r.conjugate(), r.conjugate() * ((-1 / s) * t), 1 / s), whose constructor normalises"""
    q, t, s = S
    qc = [-q[0], -q[1], -q[2], q[3]]
    k = -1 / s
    ti = P.quat_rotate(qc, [k * t[0], k * t[1], k * t[2]])
    return P.quat_normalized(qc), list(ti), 1 / s


def sim3_oplus(S, update, fix_scale):
    """VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:77-84)"""
    u = [float(x) for x in update]
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def ldlt_solve(H, b):
    """(ok, x) of H x = b for a symmetric n x n list of lists; unpivoted L D L^T, a pivot that is not > 0 fails"""
    n = len(b)
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    for j in range(n):
        d = H[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k] * D[k]
        if not d > 0.0:
            return False, None
        D[j] = d
        for i in range(j + 1, n):
            s = H[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k] * D[k]
            L[i][j] = s / d
    y = [0.0] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s
    x = [0.0] * n
    for i in reversed(range(n)):
        s = y[i] / D[i]
        for k in range(i + 1, n):
            s -= L[k][i] * x[k]
        x[i] = s
    return True, x


# ---- the edges -------------------------------------------------------------------------------------------------------------------
def camera_points(view, Xw):
    """R * P3Dw + t in cv::Mat float arithmetic (Optimizer.cc:1452, :1460): a float dot product in index order, then the addend"""
    R = np.asarray(view["Rcw"], F32).reshape(3, 3)
    t = np.asarray(view["tcw"], F32).reshape(3)
    X = np.asarray(Xw, F32).reshape(-1, 3)
    return np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)


class _Edges:
    """The 2 n edges as interleaved columns.  errors(S) = the error vectors at the estimate S (S.inverse() for the odd rows)."""

    def __init__(self, view1, view2, pairs):
        n = len(pairs)
        self.n = n
        c1 = camera_points(view1, pairs["Xw1"]).astype(np.float64)
        c2 = camera_points(view2, pairs["Xw2"]).astype(np.float64)
        self.P12, self.P21 = c2, c1                       # e12 moves P3D2c, e21 moves P3D1c
        self.obs = np.empty((2 * n, 2))
        self.obs[0::2], self.obs[1::2] = pairs["obs1"], pairs["obs2"]
        self.w = np.empty(2 * n)
        self.w[0::2], self.w[1::2] = pairs["inv_sigma2_1"], pairs["inv_sigma2_2"]
        self.K1 = [float(F32(view1[k])) for k in ("fx", "fy", "cx", "cy")]
        self.K2 = [float(F32(view2[k])) for k in ("fx", "fy", "cx", "cy")]

    @staticmethod
    def _project(T, K, Pc, obs):
        x, y, z = sim3_map(T, (Pc[:, 0], Pc[:, 1], Pc[:, 2]))
        with np.errstate(all="ignore"):
            return np.stack([obs[:, 0] - (x / z * K[0] + K[2]), obs[:, 1] - (y / z * K[1] + K[3])], 1)

    def errors(self, S):
        e = np.empty((2 * self.n, 2))
        e[0::2] = self._project(S, self.K1, self.P12, self.obs[0::2])
        e[1::2] = self._project(sim3_inverse(S), self.K2, self.P21, self.obs[1::2])
        return e

    def chi2(self, e):
        return e[:, 0] * (self.w * e[:, 0]) + e[:, 1] * (self.w * e[:, 1])

    def jacobians(self, S, fix_scale, step):
        """linearizeOplusN (base_fixed_sized_edge.hpp:152-209): column d = scalar * (e(+step e_d) - e(-step e_d)) through oplus"""
        scalar = 1 / (2 * step)
        J = np.empty((2 * self.n, 2, 7))
        for d in range(7):
            u = [0.0] * 7
            u[d] = step
            ep = self.errors(sim3_oplus(S, u, fix_scale))
            u[d] = -step
            em = self.errors(sim3_oplus(S, u, fix_scale))
            J[:, :, d] = scalar * (ep - em)
        return J


def optimize_sim3(view1, view2, pairs, s_R_t_in, th2, fix_scale, jac_step=1e-9, order_seed=None, noise=0.0):
    """Optimizer::OptimizeSim3.  view1 / view2: dicts Rcw (9), tcw (3), fx, fy, cx, cy (floats); pairs: an OPTSIM3_PAIR_DTYPE array;
    s_R_t_in: 13 floats; th2 a float.  jac_step: the step of the numeric Jacobian (g2o: 1e-9).  order_seed / noise: a stability run
    (random summation order, relative Gaussian noise on every reduction).
    Returns a dict: sRt (13 float32), sRt64 (the same before rounding), n_pairs, n_bad, n_inliers, iterations [2], bad [n] uint8,
    chi2 (per classification: [n, 2] of the correspondences it looked at, NaN for those dropped before), trace."""
    s_R_t_in = np.asarray(s_R_t_in, F32).reshape(13)
    th2 = float(F32(th2))
    delta = float(F32(math.sqrt(F32(th2))))                              # `const float deltaHuber = sqrt(th2)` (:1432)
    E = _Edges(view1, view2, pairs)
    n = E.n
    res = {"sRt": s_R_t_in.copy(), "sRt64": s_R_t_in.astype(np.float64), "n_pairs": n, "n_bad": 0, "n_inliers": 0, "iterations": [0, 0],
           "bad": np.zeros(n, np.uint8), "chi2": [], "trace": []}
    if n == 0:
        return res
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    summer = P._Summer(rng.permutation(2 * n) if rng is not None else None, noise, rng)
    S = sim3_from_floats(s_R_t_in)
    alive = np.ones(n, bool)
    for call in range(2):
        active = np.repeat(alive, 2)
        max_its = 5 if call == 0 else (10 if res["n_bad"] > 0 else 5)   # :1518, :1539-1551
        tr = {"iterations": 0, "trials": 0, "rejected": 0, "exit": "iterations"}

        def robust_chi(e):
            return float(summer(P._huber_cols(E.chi2(e), delta)[0][:, None], active)[0])

        lam, ni = 0.0, 2.0
        for it in range(max_its):
            e = E.errors(S)
            chi2 = E.chi2(e)
            current_chi = robust_chi(e)
            J = E.jacobians(S, fix_scale, jac_step)
            rho1 = P._huber_cols(chi2, delta)[1]
            ow = rho1 * E.w                                             # robustInformation = rho[1] * information
            we = (-(E.w[:, None] * e)) * rho1[:, None]                  # omega_r = -information * error; omega_r *= rho[1]
            AtO = J * ow[:, None, None]
            Hc = np.empty((2 * n, 7, 7))
            for i in range(7):
                for j in range(7):
                    Hc[:, i, j] = AtO[:, 0, i] * J[:, 0, j] + AtO[:, 1, i] * J[:, 1, j]
            bc = J[:, 0, :] * we[:, 0:1] + J[:, 1, :] * we[:, 1:2]
            H = summer(Hc.reshape(2 * n, 49), active).reshape(7, 7).tolist()
            b = summer(bc, active).tolist()
            if it == 0:                                                 # computeLambdaInit: tau * max |H_jj|
                lam = 1e-5 * max(abs(H[j][j]) for j in range(7))
                ni = 2.0
            rho, qmax = 0.0, 0
            while True:
                Hl = [row[:] for row in H]
                for j in range(7):
                    Hl[j][j] += lam
                ok2, x = ldlt_solve(Hl, b)
                tr["trials"] += 1
                if ok2:
                    trial = sim3_oplus(S, x, fix_scale)
                    temp_chi = robust_chi(E.errors(trial))
                    scale = 0.0
                    for j in range(7):
                        scale += x[j] * (lam * x[j] + b[j])             # computeScale
                    scale += 1e-3
                else:
                    temp_chi, scale = float(np.finfo(np.float64).max), 1.0
                with np.errstate(all="ignore"):
                    rho = float((np.float64(current_chi) - np.float64(temp_chi)) / np.float64(scale))
                if rho > 0 and math.isfinite(temp_chi) and ok2:
                    alpha = 1.0 - math.pow(2 * rho - 1, 3) if abs(rho) < 1e100 else -math.inf
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current_chi = temp_chi
                    S = trial
                else:
                    tr["rejected"] += 1
                    lam *= ni
                    ni *= 2
                    if not math.isfinite(lam):
                        break
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            tr["iterations"] += 1
            if qmax == 10 or rho == 0 or not math.isfinite(lam):
                tr["exit"] = "trials" if qmax == 10 else ("rho0" if rho == 0 else "lambda")
                break
        res["iterations"][call] = tr["iterations"]
        res["trace"].append(tr)
        # :1520-1537, :1553-1565, at the call's final estimate
        c = E.chi2(E.errors(S)).reshape(n, 2)
        with np.errstate(invalid="ignore"):
            now_bad = alive & ((c[:, 0] > th2) | (c[:, 1] > th2))
        res["chi2"].append(np.where(alive[:, None], c, np.nan))
        res["bad"][now_bad] = 1
        alive = alive & ~now_bad
        if call == 0:
            res["n_bad"] = int(now_bad.sum())
            if n - res["n_bad"] < 10:                                   # :1545: g2oS12 is not written
                return res
        else:
            res["n_inliers"] = int(alive.sum())
    res["sRt64"] = sim3_to_floats(S)
    res["sRt"] = res["sRt64"].astype(F32)
    return res


def tolerance(sRt_ref):
    """The parity criterion: one unit in the last place of a float at the scale of the block -- 2^-23 * s for the scale, 2^-23 for a
    rotation entry, 2^-23 * max(1, |t|_inf) for a translation entry.  Returns the 13 bounds."""
    v = np.asarray(sRt_ref, np.float64).reshape(13)
    tol = np.full(13, 2.0 ** -23)
    tol[0] *= abs(v[0])
    tol[10:] *= max(1.0, float(np.abs(v[10:]).max()))
    return tol


def min_margin(r, th2):
    """smallest |chi2 - th2| / th2 over every correspondence looked at in either classification (inf without one)"""
    m = math.inf
    for c in r["chi2"]:
        c = c[np.isfinite(c)]
        if c.size:
            m = min(m, float(np.abs(c - float(F32(th2))).min() / float(F32(th2))))
    return m


# ---- the seeded scene generator ----------------------------------------------------------------------------------------------------
def make_view(R, t, K=P.KITTI):
    return dict(Rcw=np.asarray(R, np.float64).reshape(9).astype(F32), tcw=np.asarray(t, np.float64).astype(F32), fx=F32(K["fx"]),
                fy=F32(K["fy"]), cx=F32(K["cx"]), cy=F32(K["cy"]))


def make_scene(seed, n_pairs=120, outliers=0.15, n_outliers=None, fix_scale=True, true_scale=1.0, rot=0.01, trans=0.05, ds=0.02,
               n_levels=8, scale_factor=1.2, th2=10.0):
    """Two keyframes looking at the same `n_pairs` points through two maps that differ by the similarity S12 = (true_scale, R12, t12):
    KITTI intrinsics, points 4 - 40 m in front of keyframe 1, X2c = S12^-1 X1c, each keyframe's map points in its own world frame,
    observation = projection + N(0, 0.7 px x 1.2^octave), planted outliers offset by 4 - 40 px on both axes in one of the two images
    (share `outliers`, or exactly `n_outliers`), everything rounded to float as the ABI carries it.  The input similarity is the truth
    perturbed by `rot` rad, `trans` m and a factor exp(ds) (ds ignored with a fixed scale, where the scale is exactly 1)."""
    from refactored_orb_slam2_amd._lib import OPTSIM3_PAIR_DTYPE
    rng = np.random.default_rng(seed)
    K = P.KITTI
    s_true = 1.0 if fix_scale else float(true_scale)
    R1w, t1w = P.rodrigues(rng.normal(size=3) * 0.05), rng.normal(size=3) * 0.5
    R2w, t2w = P.rodrigues(rng.normal(size=3) * 0.05), rng.normal(size=3) * 0.5
    R12, t12 = P.rodrigues(rng.normal(size=3) * 0.04), rng.normal(size=3) * 0.4
    z = rng.uniform(4, 40, n_pairs)
    u = rng.uniform(120, 1120, n_pairs)
    v = rng.uniform(40, 340, n_pairs)
    X1c = np.stack([(u - K["cx"]) * z / K["fx"], (v - K["cy"]) * z / K["fy"], z], 1)
    X2c = ((X1c - t12) @ R12) / s_true                               # R12^T (X1c - t12) / s
    Xw1 = (X1c - t1w) @ R1w
    Xw2 = (X2c - t2w) @ R2w
    oct1 = rng.integers(0, n_levels, n_pairs)
    oct2 = rng.integers(0, n_levels, n_pairs)
    sc1, sc2 = scale_factor ** oct1, scale_factor ** oct2
    obs1 = np.stack([u, v], 1) + rng.normal(size=(n_pairs, 2)) * (0.7 * sc1)[:, None]
    obs2 = np.stack([X2c[:, 0] / X2c[:, 2] * K["fx"] + K["cx"], X2c[:, 1] / X2c[:, 2] * K["fy"] + K["cy"]], 1)
    obs2 = obs2 + rng.normal(size=(n_pairs, 2)) * (0.7 * sc2)[:, None]
    if n_outliers is None:
        planted = rng.uniform(size=n_pairs) < outliers
    else:
        planted = np.zeros(n_pairs, bool)
        planted[rng.permutation(n_pairs)[:n_outliers]] = True
    off = rng.uniform(4, 40, (n_pairs, 2)) * rng.choice([-1.0, 1.0], (n_pairs, 2))
    in_first = rng.uniform(size=n_pairs) < 0.5
    obs1 = np.where((planted & in_first)[:, None], obs1 + off, obs1)
    obs2 = np.where((planted & ~in_first)[:, None], obs2 + off, obs2)
    pairs = np.zeros(n_pairs, OPTSIM3_PAIR_DTYPE)
    pairs["Xw1"], pairs["Xw2"], pairs["obs1"], pairs["obs2"] = Xw1, Xw2, obs1, obs2
    pairs["inv_sigma2_1"] = (1.0 / sc1 ** 2).astype(F32)
    pairs["inv_sigma2_2"] = (1.0 / sc2 ** 2).astype(F32)
    dr = rng.normal(size=3)
    dr *= rot / np.linalg.norm(dr)
    dt = rng.normal(size=3)
    dt *= trans / np.linalg.norm(dt)
    s_in = 1.0 if fix_scale else s_true * math.exp(ds)
    sRt_true = np.concatenate([[s_true], R12.reshape(9), t12]).astype(F32)
    sRt_in = np.concatenate([[s_in], (P.rodrigues(dr) @ R12).reshape(9), t12 + dt]).astype(F32)
    return dict(view1=make_view(R1w, t1w), view2=make_view(R2w, t2w), pairs=pairs, sRt_in=sRt_in, sRt_true=sRt_true, th2=F32(th2),
                fix_scale=bool(fix_scale), planted=planted, oct1=oct1.astype(np.int32), oct2=oct2.astype(np.int32),
                inv_level_sigma2=(1.0 / (scale_factor ** np.arange(n_levels)) ** 2).astype(F32))


# name -> (seed, keyword arguments of make_scene).  The seeds are the first ones tried (1, 2, ...): tests/test_optsim3_cpu.py asserts
# that the conditions of a parity case hold for them (margin, stability, and the counts the names promise).  second_round is the
# exception: 14 is the first seed from 13 on for which the reading drops a correspondence in the SECOND classification (a rare event
# with this generator: the first optimize() call usually converges).
CASES = {
    "fixed_scale": (1, dict()),
    "free_scale": (2, dict(fix_scale=False, true_scale=1.07)),
    "pairs_24": (3, dict(n_pairs=24, outliers=0.12)),
    "outliers_40": (4, dict(outliers=0.4, n_pairs=200)),
    "pairs_12_return_0": (5, dict(n_pairs=12, n_outliers=3)),
    "survivors_10": (6, dict(n_pairs=13, n_outliers=3)),
    "pairs_9": (7, dict(n_pairs=9, n_outliers=1)),
    "pairs_0": (8, dict(n_pairs=0)),
    "levels_12": (9, dict(n_levels=12, fix_scale=False, true_scale=0.94)),
    "beyond_cache": (10, dict(n_pairs=2100, outliers=0.1)),
    "clean": (11, dict(n_pairs=60, outliers=0.0)),
    "th2_7": (12, dict(n_pairs=80, th2=7.0, fix_scale=False, true_scale=1.02)),
    "second_round": (14, dict(n_pairs=80, outliers=0.45, rot=0.05, trans=0.4)),
}


def case_scene(name):
    seed, kw = CASES[name]
    return make_scene(seed, **kw)


def run_case(s, **kw):
    return optimize_sim3(s["view1"], s["view2"], s["pairs"], s["sRt_in"], s["th2"], s["fix_scale"], **kw)
