"""A float64 numpy reading of Optimizer::LocalBundleAdjustment (L/src/Optimizer.cc:437-760) from the edge list on, and of the parts
of g2o it runs (G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o): the yardstick of tests/test_lba_cpu.py and tests/test_lba_gpu.py.
Written from the reference's source, not from csrc/lba_internal.h, and structured differently on purpose: every edge is evaluated
as a numpy column, the blocks of the system are summed per vertex in edge order, and every trial can be solved twice --
  "schur": BlockSolver_6_3 with the points marginalised (G/core/block_solver.hpp:332-477) and a dense Cholesky of the reduced system,
  "full":  poses and points together with numpy.linalg.solve, no Schur complement.
SE3Quat, the Huber kernel and the float conventions are tests/np_pose.py's.

  EdgeSE3ProjectXYZ        G/types/sba/edge_project_xyz.cpp          (project() divides; Jacobians with divisions by z and z^2)
  EdgeStereoSE3ProjectXYZ  G/types/sba/edge_project_stereo_xyz.cpp   (`const double invz = 1.0f / z`: a double quotient)
  BaseBinaryEdge           G/core/base_binary_edge.hpp               (A = d e / d point, B = d e / d pose)
  Levenberg                G/core/optimization_algorithm_levenberg.cpp:60-176

What an edge's chi2() holds when LocalBundleAdjustment classifies it is the error its last computeActiveErrors() left there: the one
of the LAST TRIAL of the optimize() call, also a rejected one, and for a level-1 edge the last trial of round 1.  isDepthPositive()
is evaluated at the estimates.  Known liberties: Eigen::SimplicialLLT with its ordering is a dense unpivoted Cholesky here, fixed-size
products are taken in index order, and a failed factorisation leaves the estimates untouched (g2o applies the stale solution and
pops it).  A reading, unpinned.  Everything is double; inputs are the floats the ABI carries, widened."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import np_pose as NP

F32 = np.float32
TH_MONO, TH_STEREO = 5.991, 7.815                     # Optimizer.cc:669, :683 (double literals)
DELTA_MONO, DELTA_STEREO = NP.DELTA_MONO, NP.DELTA_STEREO
FIRST_ROUND_ONLY = 1
EDGE_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("u_right", "<f4"), ("inv_sigma2", "<f4")])


def _inverse3(M):
    """Eigen's 3 x 3 inverse (Eigen/src/LU/InverseImpl.h, compute_inverse<.., 3>): cofactors over the determinant"""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return M[i1][j1] * M[i2][j2] - M[i1][j2] * M[i2][j1]
    c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]
    det = (c0[0] * M[0][0] + c0[1] * M[1][0]) + c0[2] * M[2][0]
    inv = 1.0 / det
    R = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            R[j][i] = cof(i, j) * inv
    return R


def cholesky_solve(S, b):
    """(ok, x) of S x = b by L L^T, unpivoted; a pivot that is not > 0 is the failure of SimplicialLLT (info() != Success)"""
    S = np.array(S, np.float64)
    n = S.shape[0]
    for k in range(n):
        d = S[k, k]
        if not d > 0.0:
            return False, None
        lkk = math.sqrt(d)
        S[k, k] = lkk
        S[k + 1:, k] = S[k + 1:, k] / lkk
        c = S[k + 1:, k]
        S[k + 1:, k + 1:] -= np.outer(c, c)
    y = np.array(b, np.float64)
    for k in range(n):
        y[k] = y[k] / S[k, k]
        y[k + 1:] -= S[k + 1:, k] * y[k]
    for k in reversed(range(n)):
        y[k] = y[k] / S[k, k]
        y[:k] -= S[k, :k] * y[k]
    return True, y


class _Problem:
    def __init__(self, poses, fixed, points, edges, cam):
        self.n_kf, self.n_pt, self.n_e = len(poses), len(points), len(edges)
        self.fixed = np.asarray(fixed, np.uint8) != 0
        self.kf = edges["kf"].astype(np.int64)
        self.pt = edges["point"].astype(np.int64)
        self.obs = np.stack([edges["u"], edges["v"], edges["u_right"]], 1).astype(np.float64)
        self.stereo = ~(edges["u_right"] < 0)                       # Optimizer.cc:583
        self.w = edges["inv_sigma2"].astype(np.float64)
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(F32(cam[k])) for k in ("fx", "fy", "cx", "cy", "mbf"))
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.th = np.where(self.stereo, TH_STEREO, TH_MONO)
        se3 = [NP.se3_from_Tcw(T) for T in poses]
        self.Q = np.array([s[0] for s in se3]).reshape(-1, 4)
        self.T = np.array([s[1] for s in se3]).reshape(-1, 3)
        self.X = np.asarray(points, F32).astype(np.float64).reshape(-1, 3)

    def camera_points(self):
        q = self.Q[self.kf]
        X = self.X[self.pt]
        r = NP.quat_rotate((q[:, 0], q[:, 1], q[:, 2], q[:, 3]), (X[:, 0], X[:, 1], X[:, 2]))
        t = self.T[self.kf]
        return r[0] + t[:, 0], r[1] + t[:, 1], r[2] + t[:, 2]

    def errors(self):
        """computeError and chi2() of every edge at the estimates: (e [n, 3], chi2 [n], camera point)"""
        x, y, z = self.camera_points()
        with np.errstate(all="ignore"):
            mu = x / z * self.fx + self.cx
            mv = y / z * self.fy + self.cy
            invz = 1.0 / z
            su = x * invz * self.fx + self.cx
            sv = y * invz * self.fy + self.cy
            sr = su - self.bf * invz
        e = np.zeros((self.n_e, 3))
        e[:, 0] = self.obs[:, 0] - np.where(self.stereo, su, mu)
        e[:, 1] = self.obs[:, 1] - np.where(self.stereo, sv, mv)
        e[:, 2] = np.where(self.stereo, self.obs[:, 2] - sr, 0.0)
        chi2 = e[:, 0] * (self.w * e[:, 0]) + e[:, 1] * (self.w * e[:, 1])
        chi2 = np.where(self.stereo, chi2 + e[:, 2] * (self.w * e[:, 2]), chi2)
        return e, chi2, (x, y, z)

    def jacobians(self, cam_pt):
        """linearizeOplus of both edge types: A [n, 3, 3] (point), B [n, 3, 6] (pose); row 2 zero for monocular edges"""
        x, y, z = cam_pt
        fx, fy, bf, s = self.fx, self.fy, self.bf, self.stereo
        q = self.Q[self.kf]
        R = NP.quat_to_matrix((q[:, 0], q[:, 1], q[:, 2], q[:, 3]))
        with np.errstate(all="ignore"):
            z_2 = z * z
            B = np.zeros((self.n_e, 3, 6))
            B[:, 0, 0] = x * y / z_2 * fx
            B[:, 0, 1] = -(1 + (x * x / z_2)) * fx
            B[:, 0, 2] = y / z * fx
            B[:, 0, 3] = -1. / z * fx
            B[:, 0, 5] = x / z_2 * fx
            B[:, 1, 0] = (1 + y * y / z_2) * fy
            B[:, 1, 1] = -x * y / z_2 * fy
            B[:, 1, 2] = -x / z * fy
            B[:, 1, 4] = -1. / z * fy
            B[:, 1, 5] = y / z_2 * fy
            B[:, 2, 0] = np.where(s, B[:, 0, 0] - bf * y / z_2, 0.0)
            B[:, 2, 1] = np.where(s, B[:, 0, 1] + bf * x / z_2, 0.0)
            B[:, 2, 2] = np.where(s, B[:, 0, 2], 0.0)
            B[:, 2, 3] = np.where(s, B[:, 0, 3], 0.0)
            B[:, 2, 5] = np.where(s, B[:, 0, 5] - bf / z_2, 0.0)
            A = np.zeros((self.n_e, 3, 3))
            # monocular: -1. / z * tmp * R with tmp = [[fx, 0, -x / z * fx], [0, fy, -y / z * fy]]
            m = -1. / z
            t00, t02, t11, t12 = m * fx, m * (-x / z * fx), m * fy, m * (-y / z * fy)
            for c in range(3):
                mono0 = t00 * R[0][c] + t02 * R[2][c]
                mono1 = t11 * R[1][c] + t12 * R[2][c]
                st0 = -fx * R[0][c] / z + fx * x * R[2][c] / z_2
                st1 = -fy * R[1][c] / z + fy * y * R[2][c] / z_2
                A[:, 0, c] = np.where(s, st0, mono0)
                A[:, 1, c] = np.where(s, st1, mono1)
                A[:, 2, c] = np.where(s, st0 - bf * R[2][c] / z_2, 0.0)
        return A, B


def _huber_cols(chi2, delta):
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        out = ~(chi2 <= dsqr)
        rho0 = np.where(out, 2 * sq * delta - dsqr, chi2)
        rho1 = np.where(out, delta / sq, 1.0)
    return rho0, rho1


def optimize(poses, fixed, points, edges, cam, flags=0, solve="schur", order_seed=None, noise=0.0):
    """LocalBundleAdjustment from the edge list on.  poses [n_kf, 12] float32 (rows of [R | t]), fixed [n_kf] (lFixedCameras or
    mnId == 0), points [n_pt, 3] float32, edges EDGE_DTYPE [n_e] (kf / point: indices; u_right < 0: monocular), cam: dict fx fy cx cy
    mbf.  order_seed / noise: a stability run (edge summation order permuted, relative Gaussian noise on every summand).
    Returns a dict: poses [n_kf, 12] float32, points [n_pt, 3] float32, erase / dropped [n_e] uint8, rounds, iterations / trials /
    chi2_first / chi2_final per round, n_dropped, n_erase, accepts (one list of booleans per round), active_kf / active_pt of the
    last round run, margin (smallest |chi2 - th| / th over every classification)."""
    poses = np.asarray(poses, F32).reshape(-1, 12)
    points = np.asarray(points, F32).reshape(-1, 3)
    edges = np.asarray(edges, EDGE_DTYPE).reshape(-1)
    P = _Problem(poses, fixed, points, edges, cam)
    free = np.flatnonzero(~P.fixed)
    res = dict(poses=poses.copy(), points=points.copy(), erase=np.zeros(P.n_e, np.uint8), dropped=np.zeros(P.n_e, np.uint8), rounds=0,
               iterations=[0, 0], trials=[0, 0], chi2_first=[0.0, 0.0], chi2_final=[0.0, 0.0], n_dropped=0, n_erase=0,
               accepts=[[], []], margin=math.inf, active_kf=np.zeros(P.n_kf, bool), active_pt=np.zeros(P.n_pt, bool),
               round1_poses=None, round1_points=None)
    if len(free) == 0 or P.n_e == 0:
        return res
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    order = rng.permutation(P.n_e) if rng is not None else np.arange(P.n_e)
    level = np.zeros(P.n_e, bool)
    edge_chi2 = np.zeros(P.n_e)

    def classify():
        x, y, z = P.camera_points()
        with np.errstate(all="ignore"):
            res["margin"] = min(res["margin"], float(np.min(np.abs(edge_chi2 - P.th) / P.th)))
        return (edge_chi2 > P.th) | ~(z > 0.0)

    for rnd in range(2):
        robust = rnd == 0
        act = ~level
        sel = order[act[order]]                                        # the active edges in summation order
        kf_act = np.zeros(P.n_kf, bool)
        kf_act[P.kf[act]] = True
        kf_act &= ~P.fixed
        pt_act = np.zeros(P.n_pt, bool)
        pt_act[P.pt[act]] = True
        akf, apt = np.flatnonzero(kf_act), np.flatnonzero(pt_act)     # the active vertices: poses first, then points
        slot = np.full(P.n_kf, -1)
        slot[akf] = np.arange(len(akf))
        pslot = np.full(P.n_pt, -1)
        pslot[apt] = np.arange(len(apt))
        n_p, n_l = 6 * len(akf), 3 * len(apt)
        res["active_kf"], res["active_pt"] = kf_act, pt_act

        def robust_chi(chi2):
            c = _huber_cols(chi2, P.delta)[0] if robust else chi2
            c = c[sel]
            if noise:
                c = c * (1.0 + noise * rng.standard_normal(c.shape))
            return float(np.cumsum(c)[-1]) if len(c) else 0.0

        lam, ni = 0.0, 2.0
        current_chi = 0.0
        for it in range(5 if rnd == 0 else 10):
            e, chi2, cam_pt = P.errors()
            edge_chi2[act] = chi2[act]
            current_chi = robust_chi(chi2)
            if it == 0:
                res["chi2_first"][rnd] = current_chi
            A, B = P.jacobians(cam_pt)
            rho1 = _huber_cols(chi2, P.delta)[1] if robust else np.ones(P.n_e)
            ow = rho1 * P.w
            we = (-(P.w[:, None] * e)) * rho1[:, None]
            AtO, BtO = A * ow[:, None, None], B * ow[:, None, None]
            # per-edge blocks (BaseBinaryEdge::constructQuadraticForm): rows summed in index order
            Hll_e = np.einsum("nra,nrb->nrab", AtO, A)
            Hll_e = (Hll_e[:, 0] + Hll_e[:, 1]) + Hll_e[:, 2]
            Hpp_e = np.einsum("nra,nrb->nrab", BtO, B)
            Hpp_e = (Hpp_e[:, 0] + Hpp_e[:, 1]) + Hpp_e[:, 2]
            Hpl_e = np.einsum("nrb,nra->nrba", B, AtO)                # [pose row, point column]
            Hpl_e = (Hpl_e[:, 0] + Hpl_e[:, 1]) + Hpl_e[:, 2]
            bl_e = (A[:, 0, :] * we[:, 0:1] + A[:, 1, :] * we[:, 1:2]) + A[:, 2, :] * we[:, 2:3]
            bp_e = (B[:, 0, :] * we[:, 0:1] + B[:, 1, :] * we[:, 1:2]) + B[:, 2, :] * we[:, 2:3]
            if noise:
                for a in (Hll_e, Hpp_e, Hpl_e, bl_e, bp_e):
                    a *= 1.0 + noise * rng.standard_normal(a.shape)
            Hpp = np.zeros((len(akf), 6, 6))
            bp = np.zeros((len(akf), 6))
            Hll = np.zeros((len(apt), 3, 3))
            bl = np.zeros((len(apt), 3))
            Hpl = {}                                                   # (pose slot, point slot) -> 6 x 3
            for i in sel:
                l = pslot[P.pt[i]]
                Hll[l] += Hll_e[i]
                bl[l] += bl_e[i]
                s = slot[P.kf[i]]
                if s >= 0:
                    Hpp[s] += Hpp_e[i]
                    bp[s] += bp_e[i]
                    if (s, l) in Hpl:
                        Hpl[(s, l)] = Hpl[(s, l)] + Hpl_e[i]
                    else:
                        Hpl[(s, l)] = Hpl_e[i].copy()
            by_point = [[] for _ in apt]
            for (s, l) in sorted(Hpl):
                by_point[l].append(s)
            if it == 0:                                               # computeLambdaInit over every active vertex
                md = 0.0
                for s in range(len(akf)):
                    md = max(md, float(np.abs(np.diag(Hpp[s])).max()))
                for l in range(len(apt)):
                    md = max(md, float(np.abs(np.diag(Hll[l])).max()))
                lam, ni = 1e-5 * md, 2.0
            rho, qmax = 0.0, 0
            while True:
                res["trials"][rnd] += 1
                if solve == "schur":
                    ok2, xp, xl = _solve_schur(Hpp, bp, Hll, bl, Hpl, by_point, lam)
                else:
                    ok2, xp, xl = _solve_full(Hpp, bp, Hll, bl, Hpl, lam)
                Q0, T0, X0 = P.Q.copy(), P.T.copy(), P.X.copy()       # push
                if ok2:
                    for s, k in enumerate(akf):
                        q, t = NP.se3_mul(NP.se3_exp(xp[6 * s:6 * s + 6]), (list(P.Q[k]), list(P.T[k])))
                        P.Q[k], P.T[k] = q, t
                    P.X[apt] += xl.reshape(-1, 3)
                    _, chi2_t, _ = P.errors()
                    edge_chi2[act] = chi2_t[act]
                    temp_chi = robust_chi(chi2_t)
                    scale = 0.0
                    xs, bs = np.concatenate([xp, xl]), np.concatenate([bp.reshape(-1), bl.reshape(-1)])
                    for j in range(n_p + n_l):
                        scale += xs[j] * (lam * xs[j] + bs[j])        # computeScale over the whole vector
                    scale += 1e-3
                else:
                    temp_chi, scale = float(np.finfo(np.float64).max), 1.0
                with np.errstate(all="ignore"):
                    rho = float((np.float64(current_chi) - np.float64(temp_chi)) / np.float64(scale))
                good = rho > 0 and math.isfinite(temp_chi) and ok2
                res["accepts"][rnd].append(bool(good))
                if good:
                    alpha = 1.0 - math.pow(2 * rho - 1, 3) if abs(rho) < 1e100 else -math.inf
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current_chi = temp_chi
                else:
                    lam *= ni
                    ni *= 2
                    P.Q, P.T, P.X = Q0, T0, X0                         # pop
                    if not math.isfinite(lam):
                        break
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            res["iterations"][rnd] += 1
            if qmax == 10 or rho == 0 or not math.isfinite(lam):
                break
        res["chi2_final"][rnd] = current_chi
        res["rounds"] = rnd + 1
        bad = classify()
        if rnd == 0:
            res["round1_poses"] = np.stack([NP.se3_to_Tcw((list(P.Q[k]), list(P.T[k]))) for k in range(P.n_kf)])
            res["round1_points"] = P.X.astype(F32)
        if rnd == 1 or (flags & FIRST_ROUND_ONLY):
            res["erase"] = bad.astype(np.uint8)
            break
        level = bad
        res["dropped"] = bad.astype(np.uint8)
    res["n_dropped"], res["n_erase"] = int(res["dropped"].sum()), int(res["erase"].sum())
    out = poses.copy()
    for k in free:
        out[k] = NP.se3_to_Tcw((list(P.Q[k]), list(P.T[k])))
    res["poses"] = out
    pts = points.copy()
    touched = np.zeros(P.n_pt, bool)
    touched[P.pt] = True
    pts[touched] = P.X[touched].astype(F32)
    res["points"] = pts
    return res


def _solve_schur(Hpp, bp, Hll, bl, Hpl, by_point, lam):
    """BlockSolver::solve with Schur on: Hschur = (Hpp + lambda I) - sum Hpl Hll^-1 Hpl^T, upper blocks, landmark by landmark"""
    n_s, n_l = len(Hpp), len(Hll)
    S = np.zeros((6 * n_s, 6 * n_s))
    for s in range(n_s):
        S[6 * s:6 * s + 6, 6 * s:6 * s + 6] = Hpp[s] + lam * np.eye(6)
    coeff = np.zeros((n_s, 6))
    Dinv = np.zeros((n_l, 3, 3))
    for l in range(n_l):
        Dinv[l] = _inverse3(Hll[l] + lam * np.eye(3))
        D = Dinv[l]
        db = np.array([(D[r][0] * bl[l][0] + D[r][1] * bl[l][1]) + D[r][2] * bl[l][2] for r in range(3)])
        col = by_point[l]
        for a, i1 in enumerate(col):
            Bi = Hpl[(i1, l)]
            BD = np.empty((6, 3))
            for c in range(3):
                BD[:, c] = (Bi[:, 0] * D[0][c] + Bi[:, 1] * D[1][c]) + Bi[:, 2] * D[2][c]
            coeff[i1] += (Bi[:, 0] * db[0] + Bi[:, 1] * db[1]) + Bi[:, 2] * db[2]
            for i2 in col[a:]:
                Bj = Hpl[(i2, l)]
                prod = (BD[:, 0:1] * Bj[:, 0][None, :] + BD[:, 1:2] * Bj[:, 1][None, :]) + BD[:, 2:3] * Bj[:, 2][None, :]
                S[6 * i1:6 * i1 + 6, 6 * i2:6 * i2 + 6] -= prod
    bs = bp.reshape(-1) - coeff.reshape(-1)
    S = np.triu(S) + np.triu(S, 1).T                                   # the solver reads the upper triangle
    ok, xp = cholesky_solve(S, bs)
    if not ok:
        return False, None, None
    xl = np.zeros((n_l, 3))
    for l in range(n_l):
        cl = bl[l].copy()
        for i1 in by_point[l]:
            Bi, cp = Hpl[(i1, l)], -xp[6 * i1:6 * i1 + 6]
            t = Bi[0, :] * cp[0]
            for r in range(1, 6):
                t = t + Bi[r, :] * cp[r]
            cl = cl + t
        D = Dinv[l]
        xl[l] = [(D[r][0] * cl[0] + D[r][1] * cl[1]) + D[r][2] * cl[2] for r in range(3)]
    return True, xp, xl.reshape(-1)


def _solve_full(Hpp, bp, Hll, bl, Hpl, lam):
    """the whole system, poses and points together, without the Schur complement"""
    n_s, n_l = len(Hpp), len(Hll)
    n = 6 * n_s + 3 * n_l
    H = np.zeros((n, n))
    for s in range(n_s):
        U = np.triu(Hpp[s])
        H[6 * s:6 * s + 6, 6 * s:6 * s + 6] = U + np.triu(U, 1).T
    o = 6 * n_s
    for l in range(n_l):
        H[o + 3 * l:o + 3 * l + 3, o + 3 * l:o + 3 * l + 3] = Hll[l]
    for (s, l), Bm in Hpl.items():
        H[6 * s:6 * s + 6, o + 3 * l:o + 3 * l + 3] = Bm
        H[o + 3 * l:o + 3 * l + 3, 6 * s:6 * s + 6] = Bm.T
    H[np.arange(n), np.arange(n)] += lam
    b = np.concatenate([bp.reshape(-1), bl.reshape(-1)])
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return False, None, None
    x = np.linalg.solve(H, b)
    return True, x[:o], x[o:]


# ---- the parity criterion --------------------------------------------------------------------------------------------------------
def point_tolerance(X_ref):
    X = np.asarray(X_ref, np.float64).reshape(-1, 3)
    return 2.0 ** -23 * np.maximum(1.0, np.abs(X).max(axis=1))[:, None] * np.ones((1, 3))


def worst_ratio(poses, points, ref_poses, ref_points):
    """max |difference| / tolerance over every pose entry (np_pose.pose_tolerance) and every point coordinate"""
    worst = 0.0
    for T, Tr in zip(np.asarray(poses, np.float64).reshape(-1, 12), np.asarray(ref_poses, np.float64).reshape(-1, 12)):
        worst = max(worst, float((np.abs(T - Tr) / NP.pose_tolerance(Tr)).max()))
    Xr = np.asarray(ref_points, np.float64).reshape(-1, 3)
    if len(Xr):
        worst = max(worst, float((np.abs(np.asarray(points, np.float64).reshape(-1, 3) - Xr) / point_tolerance(Xr)).max()))
    return worst


# ---- the seeded scene builder ----------------------------------------------------------------------------------------------------
def make_scene(seed, n_free=6, n_fixed=3, n_points=300, mono=0.3, outliers=0.1, rot=0.004, trans=0.03, point_noise=0.05, behind=0,
               kf0_local=False, dead_kf=False, n_levels=8, scale_factor=1.2, step=0.9, u_min=20):
    """A stereo rig on KITTI intrinsics moving along a track: n_fixed older keyframes, then n_free local ones (indices in time
    order).  Every point lies 4 - 40 m ahead of the last keyframe that observes it and is observed by 2 - 6 consecutive keyframes, at
    least one of them local; observation = projection + N(0, 0.7 px x 1.2^octave); a share `mono` of the observations has u_right =
    -1; a share `outliers` is offset by 4 - 40 px x scale.  The input poses of the local keyframes are the truth perturbed by `rot`
    rad / `trans` m, the input points by `point_noise` m; everything is rounded to float as the ABI carries it.
    behind: that many points lie 0.5 - 1.5 m BEHIND their last observer, whose (monocular) observation is the projection all the same:
    a small chi2 with a negative depth.  kf0_local: the first local keyframe is fixed as well (mnId == 0).  dead_kf: every
    observation of the last local keyframe is a planted outlier.  Edges are listed point by point, keyframes ascending."""
    rng = np.random.default_rng(seed)
    cam = dict(NP.KITTI)
    n_kf = n_free + n_fixed
    fixed = np.zeros(n_kf, np.uint8)
    fixed[:n_fixed] = 1
    if kf0_local:
        fixed[n_fixed] = 1
    R_true, t_true = [], []
    pos = np.zeros(3)
    rv = np.zeros(3)
    for k in range(n_kf):                                              # camera centre pos, world-from-camera rotation rodrigues(rv)
        Rwc = NP.rodrigues(rv)
        R_true.append(Rwc.T)
        t_true.append(-Rwc.T @ pos)
        pos = pos + Rwc @ np.array([0.0, 0.0, step]) + rng.normal(size=3) * 0.02
        rv = rv + rng.normal(size=3) * 0.01
    sig = np.array([1.0 / (scale_factor ** l) ** 2 for l in range(n_levels)], F32)
    pts, rows = [], []
    for p in range(n_points):
        k = int(rng.integers(2, 7))
        k = min(k, n_kf)
        last = int(rng.integers(min(max(n_fixed if n_free else 0, k - 1), n_kf - 1), n_kf))   # the last observer is local
        first = last - k + 1
        z = rng.uniform(4, 40)
        is_behind = p < behind
        if is_behind:
            z = -rng.uniform(0.5, 1.5)
        u, v = rng.uniform(u_min, 1220), rng.uniform(20, 360)
        if is_behind:
            u, v = rng.uniform(500, 700), rng.uniform(150, 220)
        Pc = np.array([(u - cam["cx"]) * z / cam["fx"], (v - cam["cy"]) * z / cam["fy"], z])
        Pw = R_true[last].T @ (Pc - t_true[last])
        pts.append(Pw)
        for kf in range(first, last + 1):
            c = R_true[kf] @ Pw + t_true[kf]
            octave = int(rng.integers(0, n_levels))
            sc = scale_factor ** octave
            pu = c[0] / c[2] * cam["fx"] + cam["cx"] + rng.normal() * 0.7 * sc
            pv = c[1] / c[2] * cam["fy"] + cam["cy"] + rng.normal() * 0.7 * sc
            pr = c[0] / c[2] * cam["fx"] + cam["cx"] - cam["mbf"] / c[2] + rng.normal() * 0.7 * sc
            planted = rng.uniform() < outliers or (dead_kf and kf == n_kf - 1)
            off = rng.uniform(4, 40, 2) * sc * rng.choice([-1.0, 1.0], 2)
            if planted:
                pu, pv, pr = pu + off[0], pv + off[1], pr + off[0] * 0.5
            is_mono = rng.uniform() < mono or pr < 0 or (is_behind and c[2] < 0)
            rows.append((kf, p, pu, pv, -1.0 if is_mono else pr, sig[octave]))
    edges = np.array(rows, EDGE_DTYPE) if rows else np.zeros(0, EDGE_DTYPE)
    poses_true = np.stack([np.concatenate([R_true[k], t_true[k][:, None]], 1).reshape(12) for k in range(n_kf)]).astype(F32)
    poses = poses_true.copy()
    for k in range(n_kf):
        if fixed[k]:
            continue
        dr = rng.normal(size=3)
        dr *= rot / np.linalg.norm(dr)
        dt = rng.normal(size=3)
        dt *= trans / np.linalg.norm(dt)
        poses[k] = np.concatenate([NP.rodrigues(dr) @ R_true[k], (t_true[k] + dt)[:, None]], 1).reshape(12).astype(F32)
    points = (np.array(pts).reshape(-1, 3) + rng.normal(size=(n_points, 3)) * point_noise).astype(F32)
    return dict(poses=poses, fixed=fixed, points=points, edges=edges, cam=cam, poses_true=poses_true, flags=0)


# name -> (seed, keyword arguments of make_scene, flags).  Seeds: the first ones tried, from the case's number in the table x 100 on,
# for which the conditions of tests/test_lba_cpu.py hold (the counts the name promises, equal decisions in every run, the margin, half
# the parity tolerance between the runs).
CASES = {
    "standard": (100, dict(), 0),
    "one_free": (200, dict(n_free=1, n_fixed=1, n_points=8, outliers=0.0, mono=0.0), 0),
    "kf0_local": (300, dict(kf0_local=True, n_points=120), 0),
    "all_mono": (400, dict(mono=1.0, n_points=150), 0),
    "all_stereo": (500, dict(mono=0.0, n_points=150, u_min=300), 0),   # u_min: no u_right below 0
    "clean": (600, dict(outliers=0.0, n_points=150), 0),
    "outliers_30": (704, dict(outliers=0.3, dead_kf=True, n_points=200), 0),
    "rejected_step": (801, dict(rot=0.4, trans=3.0, point_noise=3.0, n_points=150), 0),
    "behind": (900, dict(behind=3, n_points=120), 0),
    "free_11": (1000, dict(n_free=11, n_fixed=2, n_points=200), 0),
    "points_1100": (1100, dict(n_free=4, n_fixed=2, n_points=1100), 0),
    "first_round_only": (1200, dict(n_points=120), FIRST_ROUND_ONLY),
    "edges_0": (1300, dict(n_points=0), 0),
    "no_free": (1400, dict(n_free=0, n_fixed=3, n_points=20), 0),
}


@functools.lru_cache(maxsize=None)
def case_scene(name):
    seed, kw, flags = CASES[name]
    s = make_scene(seed, **kw)
    s["flags"] = flags
    return s


def run_scene(s, **kw):
    return optimize(s["poses"], s["fixed"], s["points"], s["edges"], s["cam"], flags=s["flags"], **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reading of a case, computed once and shared; treat it as read-only"""
    return run_scene(case_scene(name))
