"""A float64 numpy reading of Optimizer::OptimizeEssentialGraph (L/src/Optimizer.cc:1366: the Sim3 form :760-1043, the SE3 form
:1052-1362) from the vertex and edge lists on, of the map correction behind it (:1014-1042, L/src/LoopClosing.cc:445-475) and of the
parts of g2o they run (G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o): the yardstick of tests/test_egraph_cpu.py,
tests/test_egraph_gpu.py and tests/test_egraph_dropin_cpp.py.  Written from the reference's sources, not from csrc/egraph_internal.h,
and structured differently on purpose: the transforms of all edges are numpy columns, an error is evaluated for every edge at once,
the system is a dense matrix summed edge by edge, and every trial can be solved in two ways --
  "envelope": an unpivoted block L L^T on the row envelope of the free vertices in vertex order, block row by block row,
  "dense":    numpy.linalg.solve on the whole matrix.
Sim3's constructor, exp, map, operator* and inverse are tests/np_optsim3.py's, the quaternion formulas and SE3Quat::exp
tests/np_pose.py's.

  Sim3::log                    G/types/sim3/sim3.h:128-197 (W.lu().solve(t): partial pivoting)
  EdgeSim3                     G/types/sim3/types_seven_dof_expmap.h:135-169: error (C * v1 * v2^-1).log(); G2O_SIM3_JACOBIAN is defined
                               nowhere, so the Jacobian is the numeric one of G/core/base_fixed_sized_edge.hpp:152-209 (step 1e-9)
  SE3Quat::log, inverse, adj   G/types/slam3d/se3quat.h:165-198, :114-119, :232-240
  EdgeSE3Expmap                G/types/sba/edge_se3_expmap.cpp:46-71: error (v2^-1 * C * v1).log(), Ji = (Tj^-1 Tij).adj(),
                               Jj = -(Ti^-1 Tij^-1).adj()
  Levenberg                    G/core/optimization_algorithm_levenberg.cpp:60-176 with setUserLambdaInit(1e-16)

Known liberties: Eigen::SimplicialLLT with its AMD ordering is the unpivoted Cholesky above (or LAPACK's pivoted LU in the "dense"
solve, which cannot report a non-positive pivot: it fails on a singular matrix or a non-finite solution only); fixed-size products
are taken in index order or by numpy's matmul; a failed factorisation leaves the estimates untouched (g2o applies the stale solution
and pops it); a vertex that is fixed or has no edge is reported with its input record, where the SE3 form of the reference would
report the normalised quaternion and s = 1.  A reading, unpinned.  Everything is double.

Stability.  `order_seed` permutes the order in which the edges are summed into H, b and chi2; `noise` multiplies every summand by
1 + noise * N(0, 1).  tests/test_egraph_cpu.py runs every named case four ways (envelope, dense, permuted, 4 ulp of noise), requires
the same accept / reject decisions and records the spread of the outputs in units of the library's parity criterion -- 2^-23 for a
rotation (quaternion) entry, 2^-23 max(1, |t|inf) for a translation entry, 2^-23 s for the scale.  The bound a device result must
meet is BOUND_UNITS of those units per path: 1 where the largest spread is at most a quarter, else four times the largest spread
(the kernel's summation order is a further draw from the same distribution)."""
from __future__ import annotations

import math

import numpy as np

from tests import np_optsim3 as O
from tests import np_pose as P

F32 = np.float32
EPS = 0.00001
SCALE_TOL = 1e-3                                      # kScaleTol (Optimizer.cc:1057)
LAMBDA_INIT = 1e-16                                   # setUserLambdaInit (:778, :1080)
NORMAL, LOOP_CONNECTION = 0, 1
ULP = 2.0 ** -52
UNIT = 2.0 ** -23

# The largest spread of the four runs over the named cases, in units of the criterion, measured by tests/test_egraph_cpu.py
# (test_stability_and_bound prints them), rounded up, and the bound that follows from it.  key: fix_scale
#   Sim3 form: chain6 0.90, band 315, fixed_mid 14.1, two_fixed 4.31, isolated 16.1, rejected_step 116, wide 486 -- the difference
#     quotient of step 1e-9 puts rounding noise of about 1e-7 relative into H and b, a run that differs in the last bit draws that
#     noise anew, and the long chains amplify it.  More than a quarter: the bound is four times the spread, 2.3e-4 absolute.
#   SE3 form: at most 1.9e-6 (rejected_step_se3): the bound of one unit stands.
MEASURED_SPREAD_UNITS = {False: 490.0, True: 2e-6}
BOUND_UNITS = {False: 4 * 490.0, True: 1.0}

SIM3_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])
VERTEX_DTYPE = np.dtype([("Scw", SIM3_DTYPE), ("Snc", SIM3_DTYPE), ("fixed", "<u4"), ("reserved", "<u4")])
EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("kind", "<u4")])


# ---- transforms as columns: (q = [x, y, z, w], t = [x, y, z], s), every entry a numpy column or a float -------------------------------
def _cols(rec):
    rec = np.asarray(rec)
    return [rec["q"][..., k].astype(np.float64) for k in range(4)], [rec["t"][..., k].astype(np.float64) for k in range(3)], \
        rec["s"].astype(np.float64)


def _normalized(q):
    """normalizeRotation on columns"""
    neg = np.asarray(q[3]) < 0
    q = [np.where(neg, -c, c) for c in q]
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q]


def sim3_inverse(S):
    """Sim3::inverse on columns (np_optsim3.sim3_inverse is scalar)"""
    q, t, s = S
    qc = [-q[0], -q[1], -q[2], q[3]]
    k = -1 / s
    ti = P.quat_rotate(qc, [k * t[0], k * t[1], k * t[2]])
    return _normalized(qc), list(ti), 1 / s


def _skew_products(om):
    """Omega and Omega * Omega as 3 x 3 lists of columns"""
    z = np.zeros_like(om[0])
    Om = [[z, -om[2], om[1]], [om[2], z, -om[0]], [-om[1], om[0], z]]
    Om2 = [[Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
    return Om, Om2


def lu_solve3(W, t):
    """W.lu().solve(t) for stacks: Eigen's PartialPivLU (the first largest |entry| of a column is its pivot), then the two triangular
    solves.  W: [E, 3, 3], t: [E, 3]"""
    M = np.concatenate([W, t[:, :, None]], axis=2)
    idx = np.arange(M.shape[0])
    for k in range(2):
        p = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        rows_k, rows_p = M[idx, k].copy(), M[idx, p].copy()
        M[idx, k], M[idx, p] = rows_p, rows_k
        M[:, k + 1:, k] = M[:, k + 1:, k] / M[:, k:k + 1, k]
        M[:, k + 1:, k + 1:] = M[:, k + 1:, k + 1:] - M[:, k + 1:, k:k + 1] * M[:, k:k + 1, k + 1:]
    x2 = M[:, 2, 3] / M[:, 2, 2]
    x1 = (M[:, 1, 3] - M[:, 1, 2] * x2) / M[:, 1, 1]
    x0 = (M[:, 0, 3] - M[:, 0, 1] * x1 - M[:, 0, 2] * x2) / M[:, 0, 0]
    return np.stack([x0, x1, x2], 1)


def _delta_r(R):
    return [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]


def sim3_log(S):
    """Sim3::log on columns -> [E, 7]: omega, upsilon, sigma"""
    q, t, s = S
    s = np.asarray(s, np.float64) + np.zeros_like(q[0])
    with np.errstate(all="ignore"):
        sigma = np.log(s)
        R = P.quat_to_matrix(q)
        d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1)
        dR = _delta_r(R)
        small = d > 1 - EPS
        theta = np.arccos(np.where(small, 0.0, d))
        k = np.where(small, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        om = [k * dR[0], k * dR[1], k * dR[2]]
        theta2, sigma2 = theta * theta, sigma * sigma
        tiny = np.abs(sigma) < EPS
        C = np.where(tiny, 1.0, (s - 1) / sigma)
        a, b, c = s * np.sin(theta), s * np.cos(theta), theta2 + sigma * sigma
        A = np.where(tiny, np.where(small, 1. / 2., (1 - np.cos(theta)) / theta2),
                     np.where(small, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(tiny, np.where(small, 1. / 6., (theta - np.sin(theta)) / (theta2 * theta)),
                     np.where(small, ((0.5 * sigma2 - sigma + 1) * s - 1) / (sigma2 * sigma),
                              (C - ((b - 1) * sigma + a * theta) / c) * 1 / theta2))
    Om, Om2 = _skew_products(om)
    W = np.stack([np.stack([A * Om[i][j] + B * Om2[i][j] + C * (1.0 if i == j else 0.0) for j in range(3)], 1) for i in range(3)], 1)
    ups = lu_solve3(W, np.stack(t, 1))
    return np.concatenate([np.stack(om, 1), ups, sigma[:, None]], 1)


def se3_mul(a, b):
    """SE3Quat::operator* on columns"""
    r = P.quat_rotate(a[0], b[1])
    return _normalized(P.quat_mul(a[0], b[0])), [a[1][0] + r[0], a[1][1] + r[1], a[1][2] + r[2]]


def se3_inverse(T):
    """SE3Quat::inverse: no normalisation"""
    q, t = T
    qc = [-q[0], -q[1], -q[2], q[3]]
    return qc, list(P.quat_rotate(qc, [-t[0], -t[1], -t[2]]))


def se3_log(T):
    """SE3Quat::log on columns -> [E, 6]"""
    q, t = T
    with np.errstate(all="ignore"):
        R = P.quat_to_matrix(q)
        d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1)
        dR = _delta_r(R)
        near = np.abs(d) > 0.99999
        theta = np.arccos(np.where(near, 0.0, d))
        k = np.where(near, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        c2 = np.where(near, 1. / 12., (1 - theta / (2 * np.tan(theta / 2))) / (theta * theta))
    om = [k * dR[0], k * dR[1], k * dR[2]]
    Om, Om2 = _skew_products(om)
    ups = []
    for i in range(3):
        V = [(1.0 if i == j else 0.0) - 0.5 * Om[i][j] + c2 * Om2[i][j] for j in range(3)]
        ups.append(V[0] * t[0] + V[1] * t[1] + V[2] * t[2])
    return np.stack(om + ups, 1)


def se3_adj(T):
    """SE3Quat::adj on columns -> [E, 6, 6]: [R 0; skew(t) R  R]"""
    q, t = T
    R = np.stack([np.stack(row, 1) for row in P.quat_to_matrix(q)], 1)
    z = np.zeros_like(t[0])
    sk = np.stack([np.stack([z, -t[2], t[1]], 1), np.stack([t[2], z, -t[0]], 1), np.stack([-t[1], t[0], z], 1)], 1)
    A = np.zeros((R.shape[0], 6, 6))
    A[:, :3, :3] = R
    A[:, 3:, 3:] = R
    A[:, 3:, :3] = sk @ R
    return A


# ---- the graph -----------------------------------------------------------------------------------------------------------------------
def valid(vertices, edges, fix_scale):
    """The limits of the library on the records (include/orbfe.h): True when the graph is accepted"""
    n = len(vertices)
    for rec in (vertices["Scw"], vertices["Snc"]):
        flat = np.concatenate([rec["q"].reshape(n, 4), rec["t"].reshape(n, 3), rec["s"].reshape(n, 1)], 1)
        if not np.isfinite(flat).all() or not (rec["s"] > 0).all() or not ((rec["q"] ** 2).sum(-1) > 0).all():
            return False
        if fix_scale and (np.abs(rec["s"] - 1.0) > SCALE_TOL).any():
            return False
    i, j = edges["i"], edges["j"]
    if ((i < 0) | (i >= n) | (j < 0) | (j >= n) | (i == j) | (edges["kind"] > 1)).any():
        return False
    if fix_scale and len(edges):
        loop = edges["kind"] == LOOP_CONNECTION
        si = np.where(loop, vertices["Scw"]["s"][i], vertices["Snc"]["s"][i])
        sj = np.where(loop, vertices["Scw"]["s"][j], vertices["Snc"]["s"][j])
        if (np.abs(sj * (1 / si) - 1.0) > SCALE_TOL).any():          # checkUnitScale of the derived measurement
            return False
    return True


def envelope(n_kf, fixed, edges):
    """(slot [n_kf] (-1: not in the system), first [nf], blocks): the row envelope in vertex order"""
    has = np.zeros(n_kf, bool)
    has[edges["i"]] = True
    has[edges["j"]] = True
    free = has & ~np.asarray(fixed, bool)
    slot = np.where(free, np.cumsum(free) - 1, -1)
    nf = int(free.sum())
    first = np.arange(nf)
    for e in edges:
        a, b = slot[e["i"]], slot[e["j"]]
        if a >= 0 and b >= 0:
            first[max(a, b)] = min(first[max(a, b)], min(a, b))
    return slot, first, int((np.arange(nf) - first + 1).sum())


def envelope_blocks_brute(n_kf, fixed, edges):
    """The same count from the dense pattern of H: per free row, the blocks from its first non-zero to the diagonal"""
    n_kf = int(n_kf)
    deg = np.zeros(n_kf, int)
    for e in edges:
        deg[e["i"]] += 1
        deg[e["j"]] += 1
    keep = [k for k in range(n_kf) if deg[k] > 0 and not (fixed is not None and fixed[k])]
    pos = {k: r for r, k in enumerate(keep)}
    A = np.eye(len(keep), dtype=bool)
    for e in edges:
        if e["i"] in pos and e["j"] in pos:
            A[pos[e["i"]], pos[e["j"]]] = A[pos[e["j"]], pos[e["i"]]] = True
    return int(sum(r - int(np.argmax(A[r, :r + 1])) + 1 for r in range(len(keep))))


def _solve_envelope(H, b, first, D):
    """(ok, x): unpivoted block L L^T on the row envelope, up-looking; a pivot that is not > 0 fails"""
    nf = len(first)
    L = np.zeros_like(H)
    for r in range(nf):
        rs = slice(r * D, r * D + D)
        for c in range(first[r], r):
            ks = max(first[r], first[c])
            cs = slice(c * D, c * D + D)
            B = H[rs, cs] - L[rs, ks * D:c * D] @ L[cs, ks * D:c * D].T
            L[rs, cs] = np.linalg.solve(L[cs, cs], B.T).T
        Bd = H[rs, rs] - L[rs, first[r] * D:r * D] @ L[rs, first[r] * D:r * D].T
        Ld = np.zeros((D, D))
        for j in range(D):
            d = Bd[j, j] - Ld[j, :j] @ Ld[j, :j]
            if not d > 0.0:
                return False, None
            Ld[j, j] = math.sqrt(d)
            for i in range(j + 1, D):
                Ld[i, j] = (Bd[i, j] - Ld[i, :j] @ Ld[j, :j]) / Ld[j, j]
        L[rs, rs] = Ld
    y = b.copy()
    for r in range(nf):
        rs = slice(r * D, r * D + D)
        y[rs] = np.linalg.solve(L[rs, rs], y[rs] - L[rs, first[r] * D:r * D] @ y[first[r] * D:r * D])
    for r in reversed(range(nf)):
        rs = slice(r * D, r * D + D)
        y[rs] = np.linalg.solve(L[rs, rs].T, y[rs])
        y[first[r] * D:r * D] -= L[rs, first[r] * D:r * D].T @ y[rs]
    return True, y


def _solve_dense(H, b):
    try:
        x = np.linalg.solve(H, b)
    except np.linalg.LinAlgError:
        return False, None
    return (True, x) if np.isfinite(x).all() else (False, None)


class _Graph:
    def __init__(self, vertices, edges, fix_scale):
        self.se3 = bool(fix_scale)
        self.D = 6 if self.se3 else 7
        self.i, self.j = edges["i"].astype(int), edges["j"].astype(int)
        loop = edges["kind"] == LOOP_CONNECTION
        Scw, Snc = vertices["Scw"], vertices["Snc"]

        def pick(idx):
            rec = Snc[idx].copy()
            rec[loop] = Scw[idx][loop]
            return _cols(rec)

        C = O.sim3_mul(pick(self.j), sim3_inverse(pick(self.i)))          # Sjw * Swi
        q, t, s = _cols(Scw)
        if self.se3:                                                      # SE3Quat(S.rotation(), S.translation()) normalises
            self.C = (_normalized(C[0]), C[1], np.ones(len(edges)))
            self.est = [np.stack(_normalized(q), 1), np.stack(t, 1), np.ones(len(vertices))]
        else:
            self.C = C
            self.est = [np.stack(q, 1), np.stack(t, 1), s.copy()]

    def _at(self, est, idx):
        return [est[0][idx, k] for k in range(4)], [est[1][idx, k] for k in range(3)], est[2][idx]

    def errors(self, est, Si=None, Sj=None):
        Si = self._at(est, self.i) if Si is None else Si
        Sj = self._at(est, self.j) if Sj is None else Sj
        if self.se3:
            Ti, Tj, C = (Si[0], Si[1]), (Sj[0], Sj[1]), (self.C[0], self.C[1])
            return se3_log(se3_mul(se3_mul(se3_inverse(Tj), C), Ti))      # (v2^-1 * C * v1).log()
        return sim3_log(O.sim3_mul(O.sim3_mul(self.C, Si), sim3_inverse(Sj)))   # (C * v1 * v2^-1).log()

    def jacobians(self, est, step=1e-9):
        """[E, D, D] for vertex 0 and for vertex 1 (rows: the error, columns: the update)"""
        E = len(self.i)
        Si, Sj = self._at(est, self.i), self._at(est, self.j)
        if self.se3:
            Ti, Tj, C = (Si[0], Si[1]), (Sj[0], Sj[1]), (self.C[0], self.C[1])
            return se3_adj(se3_mul(se3_inverse(Tj), C)), -se3_adj(se3_mul(se3_inverse(Ti), se3_inverse(C)))
        Ji, Jj = np.empty((E, 7, 7)), np.empty((E, 7, 7))
        scalar = 1 / (2 * step)
        for d in range(7):
            u = [0.0] * 7
            u[d] = step
            up = O.sim3_exp(u)
            u[d] = -step
            um = O.sim3_exp(u)
            Ji[:, :, d] = scalar * (self.errors(est, Si=O.sim3_mul(up, Si)) - self.errors(est, Si=O.sim3_mul(um, Si)))
            Jj[:, :, d] = scalar * (self.errors(est, Sj=O.sim3_mul(up, Sj)) - self.errors(est, Sj=O.sim3_mul(um, Sj)))
        return Ji, Jj

    def oplus(self, est, kf, x):
        """exp(x) * estimate of vertex kf"""
        S = ([float(c) for c in est[0][kf]], [float(c) for c in est[1][kf]], float(est[2][kf]))
        if self.se3:
            q, t = P.se3_mul(P.se3_exp(x), (S[0], S[1]))
            s = 1.0
        else:
            q, t, s = O.sim3_mul(O.sim3_exp(x), S)
        est[0][kf], est[1][kf], est[2][kf] = q, t, s


def essential_graph(vertices, edges, fix_scale, solve="envelope", order_seed=None, noise=0.0, jac_step=1e-9):
    """Optimizer::OptimizeEssentialGraph from the lists on.  vertices: VERTEX_DTYPE, edges: EDGE_DTYPE.  Returns a dict: sim3 (SIM3_DTYPE
    [n_kf]: the corrected Siw), poses ([n_kf, 12] float32: [R | t / s]), status (0, 1: a factorisation failed, -1: refused), iterations,
    trials, n_free, envelope_blocks, chi2_first, chi2_last, lam, decisions (one bool per trial: accepted), rhos, min_rho (the smallest
    |rho| of a trial, inf without one)."""
    vertices = np.ascontiguousarray(vertices, VERTEX_DTYPE).reshape(-1)
    edges = np.ascontiguousarray(edges, EDGE_DTYPE).reshape(-1)
    n_kf, n_e = len(vertices), len(edges)
    res = dict(sim3=vertices["Scw"].copy(), status=0, iterations=0, trials=0, n_free=0, envelope_blocks=0, chi2_first=0.0, chi2_last=0.0,
               lam=0.0, decisions=[], rhos=[], min_rho=math.inf)

    def finish():
        res["poses"] = poses_of(res["sim3"], fix_scale)
        return res

    if not valid(vertices, edges, fix_scale):
        res["status"] = -1
        return finish()
    slot, first, blocks = envelope(n_kf, vertices["fixed"] != 0, edges)
    nf = len(first)
    res["n_free"], res["envelope_blocks"] = nf, blocks
    if nf == 0 or n_e == 0:
        return finish()
    G = _Graph(vertices, edges, fix_scale)
    D = G.D
    kf_of_slot = np.flatnonzero(slot >= 0)
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    order = rng.permutation(n_e) if rng is not None else np.arange(n_e)
    nrng = np.random.default_rng(0 if order_seed is None else order_seed + 1)

    def jitter(a):
        return a * (1.0 + noise * nrng.standard_normal(np.shape(a))) if noise else a

    def chi_of(err):
        c = (err * err).sum(1)
        total = 0.0
        for e in order:
            total += float(jitter(c[e]))
        return total

    est = G.est
    lam, ni = LAMBDA_INIT, 2.0
    current_chi = 0.0
    for it in range(20):
        err = G.errors(est)
        current_chi = chi_of(err)
        if it == 0:
            res["chi2_first"] = current_chi
        Ji, Jj = G.jacobians(est, jac_step)
        H = np.zeros((nf * D, nf * D))
        b = np.zeros(nf * D)
        for e in order:
            a, c = slot[G.i[e]], slot[G.j[e]]
            A, B, w = Ji[e], Jj[e], -err[e]
            if a >= 0:
                H[a * D:a * D + D, a * D:a * D + D] += jitter(A.T @ A)
                b[a * D:a * D + D] += jitter(A.T @ w)
            if c >= 0:
                H[c * D:c * D + D, c * D:c * D + D] += jitter(B.T @ B)
                b[c * D:c * D + D] += jitter(B.T @ w)
            if a >= 0 and c >= 0:
                blk = jitter(A.T @ B)
                H[a * D:a * D + D, c * D:c * D + D] += blk
                H[c * D:c * D + D, a * D:a * D + D] += blk.T
        rho, qmax = 0.0, 0
        while True:
            Hl = H + lam * np.eye(nf * D)
            ok2, x = _solve_envelope(Hl, b, first, D) if solve == "envelope" else _solve_dense(Hl, b)
            res["trials"] += 1
            if ok2:
                backup = [a.copy() for a in est]
                for r in range(nf):
                    G.oplus(est, kf_of_slot[r], x[r * D:r * D + D])
                temp_chi = chi_of(G.errors(est))
                scale = float(np.cumsum(x * (lam * x + b))[-1]) + 1e-3      # computeScale
            else:
                res["status"] = 1
                temp_chi, scale = float(np.finfo(np.float64).max), 1.0
            with np.errstate(all="ignore"):
                rho = float((np.float64(current_chi) - np.float64(temp_chi)) / np.float64(scale))
            accepted = bool(rho > 0 and math.isfinite(temp_chi) and ok2)
            res["decisions"].append(accepted)
            res["rhos"].append(rho)
            res["min_rho"] = min(res["min_rho"], abs(rho))
            if accepted:
                alpha = 1.0 - math.pow(2 * rho - 1, 3) if abs(rho) < 1e100 else -math.inf
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current_chi = temp_chi
            else:
                if ok2:
                    est[0], est[1], est[2] = backup
                    G.est = est
                lam *= ni
                ni *= 2
                if not math.isfinite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        res["iterations"] += 1
        if qmax == 10 or rho == 0 or not math.isfinite(lam):
            break
    res["chi2_last"], res["lam"] = current_chi, lam
    out = res["sim3"]
    for k in kf_of_slot:
        out["q"][k], out["t"][k], out["s"][k] = est[0][k], est[1][k], est[2][k]
    return finish()


def poses_of(sim3, fix_scale):
    """[R | t / s] as SetPose receives them (Optimizer.cc:1003-1011; [R | t] with a fixed scale, :1324-1329), float32 [n, 12]"""
    sim3 = np.asarray(sim3, SIM3_DTYPE).reshape(-1)
    out = np.zeros((len(sim3), 12), F32)
    if not len(sim3):
        return out
    q, t, s = _cols(sim3)
    R = P.quat_to_matrix(q)
    for i in range(3):
        for j in range(3):
            out[:, 4 * i + j] = R[i][j]
        out[:, 4 * i + 3] = t[i] if fix_scale else t[i] * (1. / s)
    return out


def correct_points(points, ref, sim3_from, sim3_to):
    """correctedSwr.map(Srw.map(P)) with correctedSwr = CorrectedSiw.inverse(); ref < 0: the point goes through.  float32 [n, 3]"""
    points = np.asarray(points, F32).reshape(-1, 3)
    ref = np.asarray(ref, np.int64).reshape(-1)
    out = points.copy()
    m = ref >= 0
    if m.any():
        a = _cols(np.asarray(sim3_from, SIM3_DTYPE)[ref[m]])
        b = sim3_inverse(_cols(np.asarray(sim3_to, SIM3_DTYPE)[ref[m]]))
        X = points[m].astype(np.float64)
        out[m] = np.stack(O.sim3_map(b, O.sim3_map(a, (X[:, 0], X[:, 1], X[:, 2]))), 1).astype(F32)
    return out


# ---- the parity criterion ------------------------------------------------------------------------------------------------------------
def sim3_units(sim3, ref):
    """max |difference| over the records in units of the criterion: 2^-23 per quaternion entry, 2^-23 max(1, |t|inf) per translation
    entry, 2^-23 s for the scale"""
    sim3, ref = np.asarray(sim3, SIM3_DTYPE).reshape(-1), np.asarray(ref, SIM3_DTYPE).reshape(-1)
    if not len(ref):
        return 0.0
    uq = np.abs(sim3["q"] - ref["q"]).max() / UNIT
    ut = (np.abs(sim3["t"] - ref["t"]).max(1) / (UNIT * np.maximum(1.0, np.abs(ref["t"]).max(1)))).max()
    us = (np.abs(sim3["s"] - ref["s"]) / (UNIT * ref["s"])).max()
    return float(max(uq, ut, us))


def pose_units(poses, ref):
    """the same for [n, 12] float poses: rotation entries 2^-23, translation entries 2^-23 max(1, |t|inf)"""
    poses, ref = np.asarray(poses, np.float64).reshape(-1, 3, 4), np.asarray(ref, np.float64).reshape(-1, 3, 4)
    if not len(ref):
        return 0.0
    ur = np.abs(poses[:, :, :3] - ref[:, :, :3]).max() / UNIT
    ut = (np.abs(poses[:, :, 3] - ref[:, :, 3]).max(1) / (UNIT * np.maximum(1.0, np.abs(ref[:, :, 3]).max(1)))).max()
    return float(max(ur, ut))


def point_units(points, ref):
    points, ref = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    if not len(ref):
        return 0.0
    return float((np.abs(points - ref).max(1) / (UNIT * np.maximum(1.0, np.abs(ref).max(1)))).max())


# ---- the seeded scene generator ------------------------------------------------------------------------------------------------------
def _sim3_record(R, t, s):
    rec = np.zeros((), SIM3_DTYPE)
    rec["q"] = P.quat_normalized(P.quat_from_matrix(np.asarray(R).tolist()))      # Sim3(Matrix3, Vector3, double)
    rec["t"], rec["s"] = t, s
    return rec


def make_scene(seed, n_kf=6, band=1, fix_scale=False, drift_scale=1.1, drift_rot=0.15, drift_trans=1.5, loop_kf=0, n_corrected=1,
               old_loops=(), extra_fixed=(), isolated=(), loop_rows=(), start_noise=0.0, meas_noise=0.002, fixed=True):
    """A closed trajectory of n_kf keyframes on a circle of 10 m.  The map drifts with the keyframe index away from the loop keyframe
    `loop_kf`: by a rotation of drift_rot rad, a translation of drift_trans m and (without fix_scale) a scale of drift_scale over the
    whole trajectory.  Every keyframe's pose is the drifted one with scale 1 plus meas_noise of odometry noise; the last n_corrected
    keyframes (the current keyframe and its neighbours) also have a CorrectedSim3 entry -- the pose in the loop keyframe's frame with
    the accumulated scale, perturbed by start_noise -- and keep the drifted pose as their NonCorrectedSim3 entry.
    Edges, in the reference's order: a loop connection from every corrected keyframe to loop_kf; then per keyframe its spanning-tree
    edge to the previous keyframe that has edges, the `old_loops` (a, b) with b < a, the covisibility edges to the keyframes 2 .. band
    ids before it, and for a keyframe of `loop_rows` one covisibility edge to keyframe loop_kf + 1 (a wide row).  `isolated` keyframes
    have no edge.  Fixed: loop_kf (unless fixed is False) and extra_fixed."""
    rng = np.random.default_rng(seed)
    s_end = 1.0 if fix_scale else float(drift_scale)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    tdir = rng.normal(size=3)
    tdir /= np.linalg.norm(tdir)
    V = np.zeros(n_kf, VERTEX_DTYPE)
    span = max(1, n_kf - 1)
    for k in range(n_kf):
        ang = 2 * math.pi * k / n_kf
        Rwc = P.rodrigues(np.array([0.0, ang, 0.0])) @ P.rodrigues(rng.normal(size=3) * 0.05)
        Ow = np.array([10 * math.cos(ang), 0.3 * math.sin(3 * ang), 10 * math.sin(ang)])
        R, t = Rwc.T, -Rwc.T @ Ow                                          # the true Tcw
        f = (k - loop_kf) / span
        sk = s_end ** f
        Rg, tg = P.rodrigues(ax * drift_rot * f), tdir * drift_trans * f   # the drift of the map at keyframe k
        Rd = R @ Rg.T @ P.rodrigues(rng.normal(size=3) * meas_noise)
        td = sk * t - Rd @ tg + rng.normal(size=3) * meas_noise
        V["Scw"][k] = V["Snc"][k] = _sim3_record(Rd, td, 1.0)
        if k >= n_kf - n_corrected and k != loop_kf:
            Rc = R @ P.rodrigues(rng.normal(size=3) * (0.001 + start_noise))
            V["Scw"][k] = _sim3_record(Rc, sk * t + rng.normal(size=3) * (0.01 + 10 * start_noise), sk)
        if (fixed and k == loop_kf) or k in extra_fixed:
            V["fixed"][k] = 1
    E = []
    for k in range(n_kf - n_corrected, n_kf):
        if k != loop_kf and k not in isolated:
            E.append((k, loop_kf, LOOP_CONNECTION))
    live = [k for k in range(n_kf) if k not in isolated]
    for idx, k in enumerate(live):
        if idx > 0:
            E.append((k, live[idx - 1], NORMAL))
        for a, bb in old_loops:
            if a == k:
                E.append((a, bb, NORMAL))
        for d in range(2, band + 1):
            if idx - d >= 0:
                E.append((k, live[idx - d], NORMAL))
        if k in loop_rows and k - (loop_kf + 1) > band:
            E.append((k, loop_kf + 1, NORMAL))
    edges = np.array(E, EDGE_DTYPE) if E else np.zeros(0, EDGE_DTYPE)
    return dict(vertices=V, edges=edges, fix_scale=bool(fix_scale))


# rejected_step: with lambda starting at 1e-16 a rejected trial repeats the Gauss-Newton step, and on the Sim3 path (an exact
# Jacobian up to its quotient's noise) that step is rejected at the noise floor only, abs(rho) about 1e-8: no seed gives a mid-run rejection of
# real margin there.  rejected_step_se3 is the case that covers push / pop -- a rejection with abs(rho) >= 0.016, nine repeats, then an
# accepted trial from the restored estimates, float poses bit-equal on the device; the Sim3 case covers a far start and the trial count only.
# name -> (seed, keyword arguments of make_scene).  tests/test_egraph_cpu.py asserts for every case that the four runs of the reading
# take the same accept / reject decisions, and what the names promise.
CASES = {
    "chain6": (155, dict(n_kf=6, band=1, drift_scale=1.1)),
    "chain6_se3": (1, dict(n_kf=6, band=1, fix_scale=True)),
    "band": (2, dict(n_kf=40, band=3, n_corrected=3, old_loops=((25, 8), (31, 12)))),
    "band_se3": (2, dict(n_kf=40, band=3, n_corrected=3, old_loops=((25, 8), (31, 12)), fix_scale=True)),
    "fixed_mid": (4, dict(n_kf=12, band=2, loop_kf=5, n_corrected=2, drift_rot=0.8, drift_trans=5.0, drift_scale=1.4)),
    "fixed_mid_se3": (3, dict(n_kf=12, band=2, loop_kf=5, n_corrected=2, fix_scale=True)),
    "two_fixed": (322, dict(n_kf=10, band=2, extra_fixed=(4,))),
    "two_fixed_se3": (4, dict(n_kf=10, band=2, extra_fixed=(4,), fix_scale=True)),
    "isolated": (360, dict(n_kf=9, band=2, isolated=(4,))),
    "isolated_se3": (5, dict(n_kf=9, band=2, isolated=(4,), fix_scale=True)),
    "rejected_step": (55, dict(n_kf=10, band=2, start_noise=0.3, drift_rot=0.6)),
    "rejected_step_se3": (412, dict(n_kf=10, band=2, start_noise=0.3, drift_rot=0.6, fix_scale=True)),
    "edges_0": (7, dict(n_kf=4, isolated=(0, 1, 2, 3))),
    "no_free": (8, dict(n_kf=3, extra_fixed=(0, 1, 2))),
    "n_kf_1": (9, dict(n_kf=1, n_corrected=0)),
    "wide": (16, dict(n_kf=300, band=8, n_corrected=4, loop_rows=(120, 200, 280), drift_rot=0.02, drift_trans=0.2, drift_scale=1.02)),
    "wide_se3": (10, dict(n_kf=300, band=8, n_corrected=4, loop_rows=(120, 200, 280), fix_scale=True)),
}


def case_scene(name):
    seed, kw = CASES[name]
    return make_scene(seed, **kw)


def run_case(s, **kw):
    return essential_graph(s["vertices"], s["edges"], s["fix_scale"], **kw)
