"""A float64 numpy / plain-Python reading of Optimizer::PoseOptimization (L/src/Optimizer.cc:233-435) and of the parts of g2o it
runs (G/ = Source/ThirdParty/g2o/g2o-20241228_git/g2o): the yardstick of tests/test_pose_cpu.py and tests/test_pose_gpu.py.  Written
from the reference's source, not from csrc/pose_internal.h, and structured differently on purpose: edges are evaluated as numpy
columns, H, b and chi are accumulated SEQUENTIALLY in keypoint-index order (np.cumsum adds left to right; that is the order of g2o's
active-edge list, sorted by edge id = order of addEdge), and the chi2 PoseOptimization reads for a level-0 edge after a round is the
one the LAST TRIAL left in the edge, also when that trial was rejected (Optimizer.cc:380-384: only outliers are recomputed).

No Eigen or g2o can be built where this runs, so this is a reading, unpinned.  Known liberties: the dense
solver is an unpivoted LDL^T (Eigen::LDLT pivots on the largest diagonal element; both fail on a non-positive pivot), Eigen's
fixed-size dot products and 3 x 3 products are taken in index order.

Everything is double; inputs are the floats the ABI carries, widened."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
CHI2_MONO, CHI2_STEREO = F32(5.991), F32(7.815)                          # Optimizer.cc:363-364 (float arrays)
DELTA_MONO, DELTA_STEREO = float(F32(math.sqrt(5.991))), float(F32(math.sqrt(7.815)))   # :269-270 (const float)


# ---- SE3Quat (G/types/slam3d/se3quat.h) with Eigen's quaternion formulas ---------------------------------------------------------
def quat_from_matrix(m):
    """Eigen::Quaternion(Matrix3) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>) -> (x, y, z, w)"""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def quat_normalized(q):
    """SE3Quat::normalizeRotation (se3quat.h:251-256)"""
    if q[3] < 0:
        q = [-c for c in q]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def quat_rotate(q, v):
    """Eigen QuaternionBase::_transformVector: uv = q.vec x v; uv += uv; v + w uv + q.vec x uv.  v: three scalars or three columns"""
    x, y, z, w = q
    ux = y * v[2] - z * v[1]
    uy = z * v[0] - x * v[2]
    uz = x * v[1] - y * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return (v[0] + w * ux + (y * uz - z * uy),
            v[1] + w * uy + (z * ux - x * uz),
            v[2] + w * uz + (x * uy - y * ux))


def quat_to_matrix(q):
    """Eigen QuaternionBase::toRotationMatrix"""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def se3_from_Tcw(T12):
    """Converter::toSE3Quat (L/src/Converter.cc:36-46): the float pose widened, SE3Quat(R, t)"""
    T = [float(v) for v in np.asarray(T12, F32).reshape(12)]
    R = [[T[0], T[1], T[2]], [T[4], T[5], T[6]], [T[8], T[9], T[10]]]
    return quat_normalized(quat_from_matrix(R)), [T[3], T[7], T[11]]


def se3_to_Tcw(se3):
    """Converter::toCvMat(SE3Quat) (L/src/Converter.cc:48-70): to_homogeneous_matrix, double -> float"""
    q, t = se3
    R = quat_to_matrix(q)
    return np.array([R[0][0], R[0][1], R[0][2], t[0], R[1][0], R[1][1], R[1][2], t[1], R[2][0], R[2][1], R[2][2], t[2]], F32)


def _mat3_mul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:202-230); u = (omega, upsilon)"""
    om, up = [float(u[0]), float(u[1]), float(u[2])], [float(u[3]), float(u[4]), float(u[5])]
    theta = math.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    Om2 = _mat3_mul(Om, Om)
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if theta < 0.00001:
        a, b, c, d = 1.0, 0.5, 0.5, 1.0 / 6.0
    else:
        a = math.sin(theta) / theta
        b = (1 - math.cos(theta)) / (theta * theta)
        c = b
        d = (theta - math.sin(theta)) / math.pow(theta, 3)
    R = [[eye[i][j] + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]
    V = [[eye[i][j] + c * Om[i][j] + d * Om2[i][j] for j in range(3)] for i in range(3)]
    t = [V[i][0] * up[0] + V[i][1] * up[1] + V[i][2] * up[2] for i in range(3)]
    return quat_normalized(quat_from_matrix(R)), t


def se3_mul(a, b):
    """SE3Quat::operator* (se3quat.h:97-103)"""
    qa, ta = a
    qb, tb = b
    r = quat_rotate(qa, tb)
    return quat_normalized(quat_mul(qa, qb)), [ta[0] + r[0], ta[1] + r[1], ta[2] + r[2]]


def huber(e, delta):
    """RobustKernelHuber::robustify (G/core/robust_kernel_impl.cpp:60-74) -> (rho0, rho1, rho2)"""
    dsqr = delta * delta
    if e <= dsqr:
        return e, 1.0, 0.0
    sqrte = math.sqrt(e)
    r1 = delta / sqrte
    return 2 * sqrte * delta - dsqr, r1, -0.5 * r1 / e


def ldlt_solve(H, b):
    """(ok, x) of H x = b, H a symmetric 6 x 6 list of lists.  Unpivoted L D L^T; a pivot that is not > 0 is the failure of
    G/solvers/dense/linear_solver_dense.h:96-104 (!isPositive -> solve returns false)."""
    n = 6
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
class _Edges:
    """Columns of the edge list in keypoint-index order"""

    def __init__(self, idx, obs, stereo, Xw, w, cam):
        self.idx, self.obs, self.stereo, self.Xw, self.w = idx, obs, stereo, Xw, w
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(F32(cam[k])) for k in ("fx", "fy", "cx", "cy", "mbf"))
        self.n = len(idx)
        self.delta = np.where(stereo, DELTA_STEREO, DELTA_MONO)
        self.bound = np.where(stereo, CHI2_STEREO, CHI2_MONO).astype(F32)

    def errors(self, se3):
        """computeError of every edge at the pose: (e [n, 3] with e[:, 2] = 0 for monocular edges, chi2 [n], camera point)"""
        q, t = se3
        r = quat_rotate(q, (self.Xw[:, 0], self.Xw[:, 1], self.Xw[:, 2]))
        x, y, z = r[0] + t[0], r[1] + t[1], r[2] + t[2]          # SE3Quat::map = _r * xyz + _t
        with np.errstate(all="ignore"):
            # monocular, edge_project_xyz_onlypose.cpp:82-95: project() divides, all double
            mu = x / z * self.fx + self.cx
            mv = y / z * self.fy + self.cy
            # stereo, edge_project_stereo_xyz_onlypose.cpp:101-109: `const float invz = 1.0f / z` -- the quotient is taken in double
            # (float / double) and stored in a float
            invz = (1.0 / z).astype(F32).astype(np.float64)
            su = x * invz * self.fx + self.cx
            sv = y * invz * self.fy + self.cy
            sr = su - self.bf * invz
        e = np.zeros((self.n, 3))
        e[:, 0] = self.obs[:, 0] - np.where(self.stereo, su, mu)
        e[:, 1] = self.obs[:, 1] - np.where(self.stereo, sv, mv)
        e[:, 2] = np.where(self.stereo, self.obs[:, 2] - sr, 0.0)
        # chi2 = _error.dot(information * _error), information = invSigma2 * I
        chi2 = e[:, 0] * (self.w * e[:, 0]) + e[:, 1] * (self.w * e[:, 1])
        chi2 = np.where(self.stereo, chi2 + e[:, 2] * (self.w * e[:, 2]), chi2)
        return e, chi2, (x, y, z)

    def jacobians(self, cam_pt):
        """linearizeOplus: J [n, 3, 6] (row 2 zero for monocular edges); both edge types, all double"""
        x, y, z = cam_pt
        with np.errstate(all="ignore"):
            invz = 1.0 / z
        invz_2 = invz * invz
        fx, fy, bf = self.fx, self.fy, self.bf
        J = np.zeros((self.n, 3, 6))
        J[:, 0, 0] = x * y * invz_2 * fx
        J[:, 0, 1] = -(1 + (x * x * invz_2)) * fx
        J[:, 0, 2] = y * invz * fx
        J[:, 0, 3] = -invz * fx
        J[:, 0, 5] = x * invz_2 * fx
        J[:, 1, 0] = (1 + y * y * invz_2) * fy
        J[:, 1, 1] = -x * y * invz_2 * fy
        J[:, 1, 2] = -x * invz * fy
        J[:, 1, 4] = -invz * fy
        J[:, 1, 5] = y * invz_2 * fy
        s = self.stereo
        J[:, 2, 0] = np.where(s, J[:, 0, 0] - bf * y * invz_2, 0.0)
        J[:, 2, 1] = np.where(s, J[:, 0, 1] + bf * x * invz_2, 0.0)
        J[:, 2, 2] = np.where(s, J[:, 0, 2], 0.0)
        J[:, 2, 3] = np.where(s, J[:, 0, 3], 0.0)
        J[:, 2, 5] = np.where(s, J[:, 0, 5] - bf * invz_2, 0.0)
        return J


def _huber_cols(chi2, delta):
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        out = chi2 > dsqr
        rho0 = np.where(out, 2 * sq * delta - dsqr, chi2)
        rho1 = np.where(out, delta / sq, 1.0)
    return rho0, rho1


class _Summer:
    """Sequential sums of edge columns: in index order, or in the order / with the relative noise a stability run asks for"""

    def __init__(self, order=None, noise=0.0, rng=None):
        self.order, self.noise, self.rng = order, noise, rng

    def __call__(self, cols, active):
        sel = np.flatnonzero(active)
        if self.order is not None:
            sel = self.order[active[self.order]]
        c = cols[sel]
        if c.shape[0] == 0:
            return np.zeros(cols.shape[1:])
        s = np.cumsum(c, axis=0)[-1]              # ((c0 + c1) + c2) + ...
        if self.noise:
            s = s * (1.0 + self.noise * self.rng.standard_normal(s.shape))
        return s


def optimize_pose(keys_xy, octave, u_right, assigned, points_xyz, cam, Tcw_in, order_seed=None, noise=0.0):
    """Optimizer::PoseOptimization.  keys_xy [n, 2] float32 (mvKeysUn), octave [n], u_right [n] float32 or None (all monocular),
    assigned [n] (>= 0: index into points_xyz [m, 3] float32), cam: dict fx fy cx cy mbf (floats) + inv_level_sigma2 (float32 array,
    its length is n_levels), Tcw_in 12 floats (rows of [R | t]).  order_seed / noise: a stability run (random summation order,
    relative Gaussian noise on every reduction).
    A row whose assigned is >= m or whose octave is outside the levels is no edge (the library's documented convention).
    Returns a dict: Tcw (12 float32), n_initial, n_bad, n_inliers, rounds, iterations, outlier [n] uint8, trace (list per round)."""
    keys_xy = np.asarray(keys_xy, F32).reshape(-1, 2)
    n = keys_xy.shape[0]
    octave = np.asarray(octave, np.int64)
    assigned = np.asarray(assigned, np.int64)
    pts = np.asarray(points_xyz, F32).reshape(-1, 3)
    sig = np.asarray(cam["inv_level_sigma2"], F32)
    ur = np.full(n, -1.0, F32) if u_right is None else np.asarray(u_right, F32)
    Tcw_in = np.asarray(Tcw_in, F32).reshape(12)
    is_edge = (assigned >= 0) & (assigned < pts.shape[0]) & (octave >= 0) & (octave < len(sig))
    idx = np.flatnonzero(is_edge)
    stereo = ~(ur[idx] < 0)                                             # Optimizer.cc:279
    obs = np.stack([keys_xy[idx, 0], keys_xy[idx, 1], ur[idx]], 1).astype(np.float64)
    E = _Edges(idx, obs, stereo, pts[assigned[idx]].astype(np.float64), sig[octave[idx]].astype(np.float64), cam)
    res = {"Tcw": Tcw_in.copy(), "n_initial": int(E.n), "n_bad": 0, "n_inliers": 0, "rounds": 0, "iterations": 0,
           "outlier": np.zeros(n, np.uint8), "trace": []}
    if E.n < 3:                                                         # :357
        return res
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    summer = _Summer(rng.permutation(E.n) if rng is not None else None, noise, rng)
    outlier = np.zeros(E.n, bool)      # mvbOutlier of the edge rows = level 1
    robust = True
    edge_chi2 = np.zeros(E.n)          # the chi2 each edge's _error holds
    pose = se3_from_Tcw(Tcw_in)
    n_bad = 0
    for rnd in range(4):
        pose = se3_from_Tcw(Tcw_in)                                     # :370
        active = ~outlier                                               # initializeOptimization(0): the level-0 edges
        tr = {"iterations": 0, "trials": 0, "rejected": 0, "exit": "iterations", "n_active": int(active.sum())}

        def robust_chi(chi2):
            c = _huber_cols(chi2, E.delta)[0] if robust else chi2
            return float(summer(c[:, None], active)[0])

        lam, ni = 0.0, 2.0
        for it in range(10 if tr["n_active"] else 0):                   # optimize(10), G/core/sparse_optimizer.cpp:394-428
            e, chi2, cam_pt = E.errors(pose)
            edge_chi2[active] = chi2[active]
            current_chi = robust_chi(chi2)
            J = E.jacobians(cam_pt)
            rho1 = _huber_cols(chi2, E.delta)[1] if robust else np.ones(E.n)
            ow = rho1 * E.w                                             # robustInformation = rho[1] * information
            we = (-(E.w[:, None] * e)) * rho1[:, None]                  # omega_r = -information * error; omega_r *= rho[1]
            AtO = J * ow[:, None, None]                                 # A^T * omega, omega diagonal
            Hc = np.zeros((E.n, 6, 6))
            for i in range(6):
                for j in range(6):
                    Hc[:, i, j] = (AtO[:, 0, i] * J[:, 0, j] + AtO[:, 1, i] * J[:, 1, j]) + AtO[:, 2, i] * J[:, 2, j]
            bc = (J[:, 0, :] * we[:, 0:1] + J[:, 1, :] * we[:, 1:2]) + J[:, 2, :] * we[:, 2:3]
            H = summer(Hc.reshape(E.n, 36), active).reshape(6, 6).tolist()
            b = summer(bc, active).tolist()
            if it == 0:                                                 # computeLambdaInit: tau * max |H_jj|
                lam = 1e-5 * max(abs(H[j][j]) for j in range(6))
                ni = 2.0
            rho, qmax, terminate = 0.0, 0, False
            while True:
                Hl = [row[:] for row in H]
                for j in range(6):
                    Hl[j][j] += lam                                     # setLambda
                ok2, x = ldlt_solve(Hl, b)
                tr["trials"] += 1
                if ok2:
                    trial = se3_mul(se3_exp(x), pose)                   # oplus
                    e_t, chi2_t, _ = E.errors(trial)
                    edge_chi2[active] = chi2_t[active]
                    temp_chi = robust_chi(chi2_t)
                    scale = 0.0
                    for j in range(6):
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
                    pose = trial
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
        # classification, :374-421: outliers are recomputed at the final pose, level-0 edges keep what the last trial left
        _, chi2_final, _ = E.errors(pose)
        edge_chi2[outlier] = chi2_final[outlier]
        chi2_f = edge_chi2.astype(F32)
        outlier = chi2_f > E.bound
        n_bad = int(outlier.sum())
        if rnd == 2:
            robust = False
        tr["chi2"], tr["bound"], tr["outlier"] = chi2_f.copy(), E.bound.copy(), outlier.copy()
        res["trace"].append(tr)
        res["rounds"] += 1
        res["iterations"] += tr["iterations"]
        if E.n < 10:                                                    # :423
            break
    res["Tcw"] = se3_to_Tcw(pose)
    res["n_bad"], res["n_inliers"] = n_bad, E.n - n_bad
    res["outlier"][E.idx] = outlier
    res["edge_rows"] = E.idx
    return res


def pose_tolerance(T_ref):
    """The parity criterion: one unit in the last place of a float at the scale of the block -- 2^-23 for a rotation entry,
    2^-23 * max(1, |t|_inf) for a translation entry.  Returns the 12 bounds."""
    T = np.asarray(T_ref, np.float64).reshape(3, 4)
    tol = np.full((3, 4), 2.0 ** -23)
    tol[:, 3] *= max(1.0, float(np.abs(T[:, 3]).max()))
    return tol.reshape(12)


def poses_agree(T, T_ref):
    d = np.abs(np.asarray(T, np.float64).reshape(12) - np.asarray(T_ref, np.float64).reshape(12))
    return bool(np.all(d <= pose_tolerance(T_ref)))


# ---- the seeded scene generator (points, not images) ----------------------------------------------------------------------------
KITTI = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, mbf=386.1448)


def rodrigues(rv):
    th = float(np.linalg.norm(rv))
    if th == 0:
        return np.eye(3)
    k = np.asarray(rv, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def make_scene(seed, n_edges=1000, outliers=0.15, mono=0.3, rot=0.01, trans=0.05, n_levels=8, gap=0.35, behind=0, noise=True,
               scale_factor=1.2):
    """A frame of `n_edges` matched keypoints interleaved with unmatched rows (assigned = -1, share `gap`): KITTI intrinsics, points
    4 - 60 m in front of a true pose, observation = projection + N(0, 0.7 px x 1.2^octave), gross outliers offset by 4 - 40 px x scale
    on both axes, monocular rows with u_right = -1, everything rounded to float as the ABI carries it; the input pose = the truth
    perturbed by `rot` rad / `trans` m.  `behind` points lie behind the camera (z < 0: regular arithmetic)."""
    rng = np.random.default_rng(seed)
    cam = dict(KITTI)
    cam["inv_level_sigma2"] = np.array([1.0 / (scale_factor ** l) ** 2 for l in range(n_levels)], F32)
    R_true = rodrigues(rng.normal(size=3) * 0.05)
    t_true = rng.normal(size=3) * 0.5
    n_rows = n_edges + int(round(n_edges * gap / (1 - gap))) if n_edges else 8
    is_edge = np.zeros(n_rows, bool)
    is_edge[rng.permutation(n_rows)[:n_edges]] = True
    n_pts = n_edges + 7
    z = rng.uniform(4, 60, n_pts)
    if behind:
        z[:behind] = -rng.uniform(4, 60, behind)
    u = rng.uniform(20, 1220, n_pts)
    v = rng.uniform(20, 360, n_pts)
    Pc = np.stack([(u - cam["cx"]) * z / cam["fx"], (v - cam["cy"]) * z / cam["fy"], z], 1)
    Pw = ((Pc - t_true) @ R_true).astype(F32)                    # R^T (Pc - t)
    perm = rng.permutation(n_pts)
    assigned = np.full(n_rows, -1, np.int32)
    assigned[is_edge] = perm[:n_edges]
    octave = rng.integers(0, n_levels, n_rows).astype(np.int32)
    scale = scale_factor ** octave
    a = np.where(is_edge, assigned, 0)
    sig = 0.7 * scale if noise else np.zeros(n_rows)
    ku = u[a] + rng.normal(size=n_rows) * sig
    kv = v[a] + rng.normal(size=n_rows) * sig
    kr = u[a] - cam["mbf"] / z[a] + rng.normal(size=n_rows) * sig
    planted = is_edge & (rng.uniform(size=n_rows) < outliers)
    off = rng.uniform(4, 40, (n_rows, 2)) * scale[:, None] * rng.choice([-1.0, 1.0], (n_rows, 2))
    ku = np.where(planted, ku + off[:, 0], ku)
    kv = np.where(planted, kv + off[:, 1], kv)
    kr = np.where(planted, kr + off[:, 0] * 0.5, kr)
    is_mono = rng.uniform(size=n_rows) < mono
    kr = np.where(is_mono | (kr < 0) | ~is_edge & (rng.uniform(size=n_rows) < 0.5), -1.0, kr)
    dr = rng.normal(size=3)
    dr *= rot / np.linalg.norm(dr)
    dt = rng.normal(size=3)
    dt *= trans / np.linalg.norm(dt)
    R_in = rodrigues(dr) @ R_true
    t_in = t_true + dt
    T_true = np.concatenate([R_true, t_true[:, None]], 1).reshape(12).astype(F32)
    T_in = np.concatenate([R_in, t_in[:, None]], 1).reshape(12).astype(F32)
    return dict(keys_xy=np.stack([ku, kv], 1).astype(F32), octave=octave, u_right=kr.astype(F32), assigned=assigned, points=Pw,
                cam=cam, Tcw_in=T_in, Tcw_true=T_true, planted=planted, n_levels=n_levels)


# name -> (seed, keyword arguments of make_scene, u_right given?).  Seeds: 239 and 218 are the first seeds from 200 on whose trace has an
# edge that is an outlier after round 0 and an inlier at the end (the coverage condition); the others are the first tried.  The 9-, 3-
# and 2-edge cases have stereo rows only: three monocular edges (6 equations, some of them outliers) leave the 6-DoF pose barely
# determined, which is a property of the input, not something a parity test should sit on.
CASES = {
    "standard": (239, dict(), True),
    "all_mono": (102, dict(mono=1.0), True),
    "all_stereo": (103, dict(mono=0.0), True),
    "u_right_null": (104, dict(mono=1.0), False),
    "edges_40": (105, dict(n_edges=40), True),
    "edges_12": (106, dict(n_edges=12, outliers=0.1), True),
    "edges_9": (107, dict(n_edges=9, outliers=0.12, mono=0.0), True),
    "edges_3": (108, dict(n_edges=3, outliers=0.0, mono=0.0), True),
    "edges_2": (109, dict(n_edges=2, outliers=0.0, mono=0.0), True),
    "outliers_40": (218, dict(outliers=0.4), True),
    "large_error": (111, dict(rot=0.06, trans=0.4), True),
    "levels_12": (112, dict(n_levels=12), True),
    "behind": (113, dict(behind=5), True),
}


def case_scene(name):
    seed, kw, with_ur = CASES[name]
    s = make_scene(seed, **kw)
    if not with_ur:
        s["u_right"] = None
    return s


def run_case(s, **kw):
    return optimize_pose(s["keys_xy"], s["octave"], s["u_right"], s["assigned"], s["points"], s["cam"], s["Tcw_in"], **kw)
