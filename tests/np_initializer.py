"""The yardstick of Initializer::Initialize, written from L/src/Initializer.cc (L/ = Source/Libraries/ORB_SLAM2/) as numpy arrays over
(hypothesis, match); numpy.linalg stands where the reference calls cv::SVDecomp, cv::Mat::inv and cv::determinant.

Two modes of one code path (run(..., mode)):
  R64  everything in float64 on the float32 inputs: the truth.
  R32  float32 where the reference is float (which is everywhere but a few double intermediates), numpy.linalg.svd on float32
       matrices: what single precision does by itself.  Normalize sums in index order (cumsum), so T1 / T2 are THE float32 reading.

Margin verdicts (verdicts(r64, r32)).  A decision is a PARITY decision when R64 and R32 agree on it and its R64 value is at least a
margin away from its threshold; only those are compared exactly with the device:
  inlier test  both chi-squares are CHI_MARGIN (relative) away from their threshold
  winner       the R64 winner's score leads the runner-up by SCORE_GAP (relative) plus what the non-parity inlier tests of the two
               could move, and R32 picks it too
  RH > 0.40    |RH - 0.40| >= RH_MARGIN
  :590         both ratios of singular values are D_MARGIN away from 1.00001
  CheckRT      per inlier and candidate: every test it reaches is RT_MARGIN (relative; the cosine against 0.99998 in units of
               1 - 0.99998) away from its threshold
  acceptance   every CheckRT decision of the candidates is parity (the counts are then exact) or each count condition's slack exceeds
               the non-parity ones; the parallax condition, where it is reached, is PARALLAX_MARGIN degrees away
The reconstruction half (candidates, CheckRT, acceptance, R21 / t21 / P3D) is compared on the selection the LIBRARY made: compare()
runs reconstruct() in float64 and float32 on the library's own winning matrix and inlier verdicts, so that every named scene is
followed to its exit also where the winner is not a parity decision; where it is one, the library's selection must be the yardstick's.
A hypothesis' MATRIX (not a decision) is compared only where its null space has a gap: (s[7] - s[8]) >= NULL_GAP * s[0] for the
16x9, s[7] >= NULL_GAP * s[0] for the 8x9.
The constants were chosen on the CPU from R32 against R64 and from the host build of csrc/initializer_internal.h against R64 (they
are generous: at them R32 and the host build agree with R64 on every parity decision of every case below); they are not tuned to
device output.  NON_PARITY_CAP bounds the share of a case's decisions that may be non-parity (the figure of np_sim3.py).

Census of exits (census(r)): every `reason` bit and every CheckRT exit is reached by a directed scene of CASES, except
  NO_MODEL          needs every hypothesis of both models to score 0: reached by an engineered input in the GPU suite (H = 0), not by
                    a scene
  FEW_MATCHES       fewer than 8 matches is no scene of Tracking's (it asks for 100): reached by the N = 7 shape tests of both suites
  rt_not_finite     the triangulated point is finite for every non-degenerate 4x4; no generic scene produces one
  H_FEW_GOOD        bestGood <= 0.9 N with the other three conditions of :710-711 reached is a plane whose inliers fail CheckRT in
                    numbers; the scenes tried end in the F model first.  The rule itself is covered on engineered counts
                    (tests/test_initializer_cpu.py: the decision functions of the host build)
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
NULL_GAP, CHI_MARGIN, SCORE_GAP, RH_MARGIN, RT_MARGIN, PARALLAX_MARGIN, D_MARGIN = 1e-4, 1e-2, 1e-3, 0.02, 1e-2, 0.05, 5e-6
NON_PARITY_CAP = 0.03
(FEW_MATCHES, NO_MODEL, H_DEGENERATE, F_FEW_GOOD, F_SIMILAR, F_PARALLAX, H_SECOND, H_PARALLAX, H_MIN_TRIANGULATED,
 H_FEW_GOOD) = (1 << k for k in range(10))
RT_EXITS = ("rt_not_finite", "rt_behind1", "rt_behind2", "rt_reproj1", "rt_reproj2", "rt_good_low_parallax", "rt_good")


def match_list(matches12):
    i1 = np.flatnonzero(np.asarray(matches12) >= 0)
    return i1, np.asarray(matches12)[i1]


def normalize(keys, f):
    """Normalize (:739-783): returns T and the normalised points; R32 sums in index order"""
    k = np.asarray(keys, F32).astype(f)
    n = len(k)
    total = (lambda v: np.cumsum(v, dtype=f)[-1]) if f is F32 else (lambda v: v.sum())
    mean = np.array([total(k[:, 0]), total(k[:, 1])], f) / f(n)
    c = k - mean
    dev = np.array([total(np.abs(c[:, 0])), total(np.abs(c[:, 1]))], f) / f(n)
    s = (1.0 / dev.astype(F64)).astype(f)
    T = np.eye(3, dtype=f)
    T[0, 0], T[1, 1], T[0, 2], T[1, 2] = s[0], s[1], -mean[0] * s[0], -mean[1] * s[1]
    return T, c * s, np.concatenate([mean, s])


def _systems(p1, p2):
    """A of ComputeH21 (H, 16, 9) and of ComputeF21 (H, 8, 9) from (H, 8, 2) normalised points"""
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    even = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
    odd = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
    AH = np.stack([even, odd], 2).reshape(len(u1), 16, 9)
    AF = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], -1)
    return AH, AF


def check_homography(H21, H12, m, sigma, f):
    """(H, 3, 3) x (N, 4) -> chi1, chi2 (H, N) (:327-376)"""
    u1, v1, u2, v2 = (m[:, k][None, :] for k in range(4))
    inv = f(1.0 / (F64(sigma) * F64(sigma)))
    g = lambda M, r, c: M[:, r, c][:, None]
    w = 1.0 / (g(H12, 2, 0) * u2 + g(H12, 2, 1) * v2 + g(H12, 2, 2))
    a = (g(H12, 0, 0) * u2 + g(H12, 0, 1) * v2 + g(H12, 0, 2)) * w
    b = (g(H12, 1, 0) * u2 + g(H12, 1, 1) * v2 + g(H12, 1, 2)) * w
    chi1 = ((u1 - a) ** 2 + (v1 - b) ** 2) * inv
    w = 1.0 / (g(H21, 2, 0) * u1 + g(H21, 2, 1) * v1 + g(H21, 2, 2))
    a = (g(H21, 0, 0) * u1 + g(H21, 0, 1) * v1 + g(H21, 0, 2)) * w
    b = (g(H21, 1, 0) * u1 + g(H21, 1, 1) * v1 + g(H21, 1, 2)) * w
    chi2 = ((u2 - a) ** 2 + (v2 - b) ** 2) * inv
    return chi1.astype(f), chi2.astype(f)


def check_fundamental(F21, m, sigma, f):
    """(H, 3, 3) x (N, 4) -> chi1, chi2 (H, N) (:405-456)"""
    u1, v1, u2, v2 = (m[:, k][None, :] for k in range(4))
    inv = f(1.0 / (F64(sigma) * F64(sigma)))
    g = lambda r, c: F21[:, r, c][:, None]
    a2, b2, c2 = g(0, 0) * u1 + g(0, 1) * v1 + g(0, 2), g(1, 0) * u1 + g(1, 1) * v1 + g(1, 2), g(2, 0) * u1 + g(2, 1) * v1 + g(2, 2)
    num2 = a2 * u2 + b2 * v2 + c2
    chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv
    a1, b1, c1 = g(0, 0) * u2 + g(1, 0) * v2 + g(2, 0), g(0, 1) * u2 + g(1, 1) * v2 + g(2, 1), g(0, 2) * u2 + g(1, 2) * v2 + g(2, 2)
    num1 = a1 * u1 + b1 * v1 + c1
    chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv
    return chi1.astype(f), chi2.astype(f)


def _scores(chi1, chi2, th, th_score, f):
    with np.errstate(invalid="ignore"):
        t1 = np.where(chi1 > th, f(0), th_score - chi1).astype(f)
        t2 = np.where(chi2 > th, f(0), th_score - chi2).astype(f)
        inl = ~(chi1 > th) & ~(chi2 > th)
    terms = np.stack([t1, t2], -1).reshape(len(chi1), -1)   # in the order the loop adds them
    score = np.cumsum(terms, axis=1, dtype=f)[:, -1] if terms.shape[1] else np.zeros(len(chi1), f)
    return score, inl


def first_max(score):
    """`currentScore > score` from 0: the first maximum, -1 when nothing is positive (NaN never wins)"""
    s = np.where(np.isnan(score), -1.0, score)
    if not len(s) or not (s > 0).any():
        return -1
    return int(np.argmax(s))


def decompose_e(E):
    u, w, vt = np.linalg.svd(E)
    t = u[:, 2] / np.linalg.norm(u[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], E.dtype)
    R1, R2 = u @ W @ vt, u @ W.T @ vt
    if np.linalg.det(R1) < 0:
        R1 = -R1
    if np.linalg.det(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def faugeras(H21, K, f):
    """ReconstructH :577-678 -> the eight (R, t), or None at the exit of :590"""
    A = np.linalg.inv(K) @ H21 @ K
    U, w, Vt = np.linalg.svd(A)
    s = f(np.linalg.det(U) * np.linalg.det(Vt))
    d1, d2, d3 = (f(x) for x in w)
    ratios = (F64(d1 / d2), F64(d2 / d3))
    if ratios[0] < 1.00001 or ratios[1] < 1.00001:
        return None, ratios
    aux1, aux3 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    ast = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [ast, -ast, -ast, ast]
    asp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [asp, -asp, -asp, asp]
    out = []
    for i in range(4):
        Rp = np.eye(3, dtype=f)
        Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[i], st[i], ct
        t = U @ (np.array([x1[i], 0, -x3[i]], f) * (d1 - d3))
        out.append(((s * U @ Rp @ Vt).astype(f), (t / np.linalg.norm(t)).astype(f)))
    for i in range(4):
        Rp = np.eye(3, dtype=f)
        Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[i], -1, sp[i], -cp
        t = U @ (np.array([x1[i], 0, x3[i]], f) * (d1 + d3))
        out.append(((s * U @ Rp @ Vt).astype(f), (t / np.linalg.norm(t)).astype(f)))
    return out, ratios


def check_rt(R, t, K, m, inl, th2, f):
    """CheckRT (:785-899) over the match list m (N, 4): per match the exit (index into RT_EXITS, -1 not an inlier), the point, the
    cosine, the margin verdict; nGood and the parallax"""
    N = len(m)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    P1 = np.zeros((3, 4), f)
    P1[:, :3] = K
    P2 = (K @ np.concatenate([R, t[:, None]], 1)).astype(f)
    O2 = (-R.T @ t).astype(f)
    x1, y1, x2, y2 = (m[:, k:k + 1] for k in range(4))
    A = np.stack([x1 * P1[2] - P1[0], y1 * P1[2] - P1[1], x2 * P2[2] - P2[0], y2 * P2[2] - P2[1]], 1).astype(f)
    vt = np.linalg.svd(A)[2] if N else np.zeros((0, 4, 4), f)
    with np.errstate(all="ignore"):
        p = (vt[:, 3, :3] / vt[:, 3, 3:4]).astype(f)
        n2 = p - O2
        d1, d2 = np.linalg.norm(p, axis=1), np.linalg.norm(n2, axis=1)
        cos = ((p * n2).sum(1) / (d1 * d2)).astype(f)
        q = (p @ R.T + t).astype(f)
        e1 = ((fx * p[:, 0] / p[:, 2] + cx - m[:, 0]) ** 2 + (fy * p[:, 1] / p[:, 2] + cy - m[:, 1]) ** 2).astype(f)
        e2 = ((fx * q[:, 0] / q[:, 2] + cx - m[:, 2]) ** 2 + (fy * q[:, 1] / q[:, 2] + cy - m[:, 3]) ** 2).astype(f)
        low = cos.astype(F64) < 0.99998
        clear_cos = np.abs(cos.astype(F64) - 0.99998) >= RT_MARGIN * (1 - 0.99998)
        code = np.full(N, -1)
        clear = np.ones(N, bool)
        live = np.asarray(inl, bool).copy()

        def exit_(cond, k):
            nonlocal live
            code[live & cond] = k
            live = live & ~cond

        exit_(~np.isfinite(p).all(1), 0)
        clear &= ~live | ((np.abs(p[:, 2]) >= RT_MARGIN * d1) & (clear_cos | (p[:, 2] > 0)))
        exit_((p[:, 2] <= 0) & low, 1)
        clear &= ~live | ((np.abs(q[:, 2]) >= RT_MARGIN * d2) & (clear_cos | (q[:, 2] > 0)))
        exit_((q[:, 2] <= 0) & low, 2)
        clear &= ~live | (np.abs(e1 - th2) >= RT_MARGIN * th2)
        exit_(e1 > th2, 3)
        clear &= ~live | (np.abs(e2 - th2) >= RT_MARGIN * th2)
        exit_(e2 > th2, 4)
        clear &= ~live | clear_cos
        code[live & ~low], code[live & low] = 5, 6
    good = code >= 5
    n_good = int(good.sum())
    parallax = f(0)
    if n_good:
        c = np.sort(cos[good])[min(50, n_good - 1)]
        parallax = f(F64(f(np.arccos(c)) * f(180)) / np.pi)
    return {"code": code, "p": p, "cos": cos, "clear": clear | (code < 0), "n_good": n_good, "parallax": parallax, "R": R, "t": t}


def run(keys1, keys2, matches12, sets, params, mode):
    """Initialize (:45-122) and what it calls, in float64 (mode 'R64') or float32 (mode 'R32')"""
    f = F64 if mode == "R64" else F32
    fx, fy, cx, cy, sigma, min_parallax, min_tri = params
    keys1, keys2 = np.asarray(keys1, F32).reshape(-1, 2), np.asarray(keys2, F32).reshape(-1, 2)
    i1, i2 = match_list(matches12)
    N, sets = len(i1), np.asarray(sets, np.int64).reshape(-1, 8)
    H = len(sets)
    r = {"mode": mode, "N": N, "i1": i1, "m": None, "K": None, "model": 0, "success": False, "reason": 0, "best_h": -1, "best_f": -1, "cands": [], "n_inliers": 0,
         "P3D": np.zeros((len(keys1), 3), f), "triangulated": np.zeros(len(keys1), bool), "R21": None, "t21": None, "exits": set(), "min_parallax": min_parallax}
    if N < 8:
        r["reason"] = FEW_MATCHES
        return r
    T1, pn1, r["norm1"] = normalize(keys1, f)
    T2, pn2, r["norm2"] = normalize(keys2, f)
    r["T1"], r["T2"] = T1, T2
    m = np.concatenate([keys1[i1], keys2[i2]], 1).astype(f)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f)
    r["m"], r["K"] = m, K
    ok = np.array([(0 <= s).all() and (s < N).all() and len(set(s.tolist())) == 8 for s in sets], bool) if H else np.zeros(0, bool)
    safe = np.where(ok[:, None], sets, np.arange(8)[None, :]) if H else sets
    AH, AF = _systems(pn1[i1][safe], pn2[i2][safe])
    uh, sh, vth = np.linalg.svd(AH) if H else (None, np.zeros((0, 9), f), np.zeros((0, 9, 9), f))
    uf, sf, vtf = np.linalg.svd(AF) if H else (None, np.zeros((0, 8), f), np.zeros((0, 9, 9), f))
    Hn, Fpre = vth[:, 8].reshape(-1, 3, 3), vtf[:, 8].reshape(-1, 3, 3)
    H21 = (np.linalg.inv(T2) @ Hn @ T1).astype(f)
    with np.errstate(all="ignore"):
        det = np.linalg.det(H21.astype(F64)) if H else np.zeros(0)
        H12 = np.where((det != 0)[:, None, None], np.linalg.inv(np.where((det != 0)[:, None, None], H21, np.eye(3, dtype=f))), f(0)).astype(f)
    u, w, vt = np.linalg.svd(Fpre) if H else (np.zeros((0, 3, 3), f),) * 3
    if H:
        w = w.copy()
        w[:, 2] = 0
    Fn = (u * w[:, None, :]) @ vt if H else np.zeros((0, 3, 3), f)
    F21 = (T2.T @ Fn @ T1).astype(f)
    with np.errstate(all="ignore"):
        c1h, c2h = check_homography(H21, H12, m, sigma, f)
        c1f, c2f = check_fundamental(F21, m, sigma, f)
    SHs, inl_h = _scores(c1h, c2h, f(5.991), f(5.991), f)
    SFs, inl_f = _scores(c1f, c2f, f(3.841), f(5.991), f)
    SHs, SFs = np.where(ok, SHs, f(0)), np.where(ok, SFs, f(0))
    inl_h, inl_f = inl_h & ok[:, None], inl_f & ok[:, None]
    r.update(ok=ok, H21=H21, F21=F21, score_h=SHs, score_f=SFs, inl_h=inl_h, inl_f=inl_f, chi_h=(c1h, c2h), chi_f=(c1f, c2f),
             sv_h=sh, sv_f=sf)
    bh, bf = first_max(SHs), first_max(SFs)
    r["best_h"], r["best_f"] = bh, bf
    SH, SF = (SHs[bh] if bh >= 0 else f(0)), (SFs[bf] if bf >= 0 else f(0))
    if bh < 0 and bf < 0:
        r["reason"] = NO_MODEL   # the reference divides 0 by 0 and passes an empty matrix on
        return r
    RH = f(SH / (SH + SF))
    r["rh"] = RH
    if F64(RH) > 0.40:
        r["model"], M, inl = 1, H21[bh], inl_h[bh]
    else:
        r["model"], M, inl = 2, F21[bf], inl_f[bf]
    r.update(reconstruct(r["model"], M, inl, m, K, i1, len(keys1), params, f))
    return r


def reconstruct(model, M, inl, m, K, i1, n1, params, f):
    """ReconstructH (:562-721) or ReconstructF (:461-560) from the chosen model's matrix M and its inlier verdicts over the match list
    m (N, 4), in dtype f: the candidates with CheckRT's outcome, the acceptance rules, and what Initialize hands back.  Separate from
    run() so that it can also be applied to a selection that is not the yardstick's own."""
    sigma, min_parallax, min_tri = params[4], params[5], params[6]
    M, K, m = np.asarray(M).reshape(3, 3).astype(f), np.asarray(K).astype(f), np.asarray(m).astype(f)
    inl = np.asarray(inl, bool)
    r = {"model": model, "inliers": inl, "n_inliers": int(inl.sum()), "cands": [], "exits": set(), "reason": 0, "success": False,
         "P3D": np.zeros((n1, 3), f), "triangulated": np.zeros(n1, bool), "R21": None, "t21": None, "min_parallax": min_parallax}
    th2 = f(4.0 * F64(f(sigma) * f(sigma)))
    if model == 1:
        cands, r["d_ratios"] = faugeras(M, K, f)
        if cands is None:
            r["reason"] = H_DEGENERATE
            return r
    else:
        cands = decompose_e((K.T @ M @ K).astype(f))
    C = [check_rt(R.astype(f), t.astype(f), K, m, inl, th2, f) for R, t in cands]
    r["cands"] = C
    for c in C:
        r["exits"] |= {RT_EXITS[k] for k in np.unique(c["code"][c["code"] >= 0])}
    g = [c["n_good"] for c in C]
    Nin = r["n_inliers"]
    if r["model"] == 2:   # :497-559
        max_good = max(g)
        n_min_good = max(int(0.9 * Nin), int(min_tri))
        nsimilar = sum(1 for x in g if x > 0.7 * max_good)
        best = g.index(max_good)
        reason = (F_FEW_GOOD if max_good < n_min_good else 0) | (F_SIMILAR if nsimilar > 1 else 0)
        if not reason and not (C[best]["parallax"] > f(min_parallax)):
            reason = F_PARALLAX
        r.update(best_candidate=best, n_good=max_good, second=nsimilar, parallax_decides=not (reason & (F_FEW_GOOD | F_SIMILAR)),
                 slack={F_FEW_GOOD: abs(max_good - n_min_good), F_SIMILAR: min(abs(x - 0.7 * max_good) for x in g)})
    else:                 # :680-720
        best_good, second, best = 0, 0, -1
        for i, x in enumerate(g):
            if x > best_good:
                second, best_good, best = best_good, x, i
            elif x > second:
                second = x
        par = C[best]["parallax"] if best >= 0 else f(-1)
        reason = ((0 if second < 0.75 * best_good else H_SECOND) | (0 if par >= f(min_parallax) else H_PARALLAX) |
                  (0 if best_good > min_tri else H_MIN_TRIANGULATED) | (0 if best_good > 0.9 * Nin else H_FEW_GOOD))
        r.update(best_candidate=best, n_good=best_good, second=second, parallax_decides=True,
                 slack={H_SECOND: abs(second - 0.75 * best_good), H_MIN_TRIANGULATED: abs(best_good - min_tri),
                        H_FEW_GOOD: abs(best_good - 0.9 * Nin)})
    r["reason"], r["success"] = reason, reason == 0
    r["parallax"] = C[r["best_candidate"]]["parallax"] if r["best_candidate"] >= 0 else f(-1)
    if r["success"]:
        w = C[r["best_candidate"]]
        good = w["code"] >= 5
        r["P3D"][i1[good]] = w["p"][good]
        r["triangulated"][i1[w["code"] == 6]] = True
        r["R21"], r["t21"] = w["R"], w["t"]
    return r


def rt_verdicts(a64, a32):
    """Parity of what reconstruct() decided, from its float64 and float32 runs on the same selection: per candidate the CheckRT
    decisions (in the order of a64's candidates), whether the acceptance is a parity decision, and the non-parity count"""
    v = {"rt": [], "decide": False, "n_dec": 1, "n_non": 1, "mask": -1}
    if a64["cands"] and len(a64["cands"]) == len(a32["cands"]):
        order = match_candidates(a64["cands"], a32["cands"])
        loose = 0
        for c, j in zip(a64["cands"], order):
            par = c["clear"] & (c["code"] == a32["cands"][j]["code"])
            v["rt"].append(par)
            v["n_dec"] += int((c["code"] >= 0).sum())
            v["n_non"] += int((~par).sum())
            loose += int((~par).sum())
        slack_ok = loose == 0 or all(s_ > loose for s_ in a64["slack"].values())   # with every CheckRT decision parity the counts are exact
        par_ok = (not a64["parallax_decides"]) or abs(F64(a64["parallax"]) - F64(a64["min_parallax"])) >= PARALLAX_MARGIN
        g = sorted((c["n_good"] for c in a64["cands"]), reverse=True)
        if a64["model"] == 1 and g[0] - g[1] <= loose:
            # ReconstructH keeps the FIRST candidate with the best count, and the order of the candidates hangs on the signs of the
            # singular vectors: with tied counts bestParallax is any of the tied candidates', in the reference as here.  H_SECOND is set
            # whichever it is; the parallax bit is not a decision of this input
            v["mask"], par_ok = ~H_PARALLAX, True
        v["decide"] = bool(slack_ok and par_ok and a64["reason"] == a32["reason"])
    elif not a64["cands"] and not a32["cands"] and "d_ratios" in a64:   # the exit of :590
        v["decide"] = bool(a64["reason"] == a32["reason"] and min(abs(x - 1.00001) for x in a64["d_ratios"]) >= D_MARGIN)
    v["n_non"] -= int(v["decide"])
    return v


def census(r):
    """the exits a run reached: its reason bits by name, 'success', and CheckRT's exits"""
    names = ["few_matches", "no_model", "h_degenerate", "f_few_good", "f_similar", "f_parallax", "h_second", "h_parallax",
             "h_min_triangulated", "h_few_good"]
    out = {names[k] for k in range(10) if r["reason"] >> k & 1} | set(r["exits"])
    if r["success"]:
        out.add("success_h" if r["model"] == 1 else "success_f")
    return out


def verdicts(r64, r32):
    """The parity masks of a case and the share of non-parity decisions"""
    v = {"share": 0.0, "hyp_h": np.zeros(0, bool), "hyp_f": np.zeros(0, bool), "model": r64["model"] == r32["model"], "win_h": False,
         "win_f": False, "decide": False, "rt": []}
    if "ok" not in r64:
        v["decide"] = r64["reason"] == r32["reason"]
        return v
    sh, sf, ok = r64["sv_h"], r64["sv_f"], r64["ok"]
    unclear = {}
    with np.errstate(all="ignore"):
        # a hypothesis whose MATRIX can be compared: the smallest singular value is separated from the next
        v["hyp_h"] = ok & (sh[:, 7] - sh[:, 8] >= NULL_GAP * sh[:, 0])
        v["hyp_f"] = ok & (sf[:, 7] >= NULL_GAP * sf[:, 0])
        for k, th in (("h", 5.991), ("f", 3.841)):
            c1, c2 = r64["chi_" + k]
            clear = (np.abs(c1 - th) >= CHI_MARGIN * th) & (np.abs(c2 - th) >= CHI_MARGIN * th)
            v["inl_" + k] = (clear & (r64["inl_" + k] == r32["inl_" + k])) | ~ok[:, None]
            unclear[k] = (~v["inl_" + k]).sum(1)
    n_dec = v["inl_h"].size + v["inl_f"].size
    n_non = n_dec - int(v["inl_h"].sum()) - int(v["inl_f"].sum())
    for k in ("h", "f"):
        s, b = r64["score_" + k], r64["best_" + k]
        if b < 0:
            v["win_" + k] = r32["best_" + k] < 0
        else:   # the lead must survive every non-parity inlier decision of the winner and of a rival: a flip moves a score by < 2 x 5.991
            rest, ur = np.delete(s, b), np.delete(unclear[k], b)
            lead = s[b] - (rest.max() if len(rest) else 0.0)
            need = SCORE_GAP * s[b] + 2 * 5.991 * (unclear[k][b] + (ur.max() if len(ur) else 0))
            v["win_" + k] = bool(lead >= need and r32["best_" + k] == b)
    v["model"] = bool(r64["model"] == r32["model"] and (r64["model"] == 0 or abs(F64(r64["rh"]) - 0.40) >= RH_MARGIN))
    n_dec += 3
    n_non += 3 - int(v["win_h"]) - int(v["win_f"]) - int(v["model"])
    win = v["model"] and (v["win_h"] if r64["model"] == 1 else v["win_f"])
    if win and r64["model"]:
        w = rt_verdicts(r64, r32)
        v["rt"], v["decide"] = w["rt"], w["decide"]
        n_dec, n_non = n_dec + w["n_dec"], n_non + w["n_non"]
    v["share"] = n_non / max(n_dec, 1)
    return v


def match_candidates(ref, got):
    """for each candidate of `ref` the index of the nearest (R, t) of `got`; asserts the assignment is one to one"""
    order = []
    for c in ref:
        d = [np.abs(np.asarray(g["R"], F64) - c["R"]).max() + np.abs(np.asarray(g["t"], F64) - c["t"]).max() for g in got]
        order.append(int(np.argmin(d)))
    assert sorted(order) == list(range(len(ref))), f"candidates do not pair one to one: {order}"
    return order


# ---- the seeded scene builder
def look_at(yaw, pitch=0.0):
    cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])


def scene(seed, kind="general", N=300, n_extra=40, outliers=0.0, noise=0.3, baseline=0.4, tilt=0.15):
    """Two views of N points: returns keys1, keys2, matches12, params, truth.  kind: 'general' (depth 4 .. 12), 'plane', 'short'
    (baseline too short for one degree), 'identical' (the same key list twice), 'forward' (a motion along the optical axis of a
    shallow scene: two similar candidates).  n_extra unmatched keypoints are interleaved in both frames, so n1 != n2 != N."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 520.0, 525.0, 320.0, 240.0
    X = np.stack([rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(4, 12, N)], 1)
    R, t = look_at(0.05, -0.02), np.array([-baseline, 0.03, 0.05])
    if kind == "plane":
        X[:, 2] = 8.0 + tilt * X[:, 0] - 0.1 * X[:, 1]
    elif kind == "short":
        t = t * 0.01
    elif kind == "identical":
        R, t = np.eye(3), np.zeros(3)
        noise = 0.0
    elif kind == "forward":
        X[:, 2] = rng.uniform(40, 41, N)
        R, t = np.eye(3), np.array([0.0, 0.0, 0.3])
    proj = lambda Y: np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1)
    a, b = proj(X), proj(X @ R.T + t)
    a, b = a + rng.normal(0, noise, a.shape), b + (rng.normal(0, noise, b.shape) if kind != "identical" else 0.0)
    if kind == "identical":
        b = a.copy()
    n_out = int(round(outliers * N))
    if n_out:
        b[rng.choice(N, n_out, replace=False)] = np.stack([rng.uniform(0, 640, n_out), rng.uniform(0, 480, n_out)], 1)
    n1, n2 = N + n_extra, N + 2 * n_extra
    slots1, slots2 = np.sort(rng.choice(n1, N, replace=False)), rng.permutation(n2)[:N]
    keys1 = np.stack([rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)], 1)
    keys2 = np.stack([rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)], 1)
    keys1[slots1], keys2[slots2] = a, b
    matches12 = np.full(n1, -1, np.int32)
    matches12[slots1] = slots2
    return (keys1.astype(F32), keys2.astype(F32), matches12, (fx, fy, cx, cy, 1.0, 1.0, 50), {"R": R, "t": t / max(np.linalg.norm(t), 1e-30)})


# name -> (scene arguments, seed of the sets); N = 300 matches, H = 64 hypotheses
CASES = {
    "general": (dict(seed=11, kind="general"), 1),
    "plane": (dict(seed=12, kind="plane"), 2),
    "outliers40": (dict(seed=13, kind="general", outliers=0.4), 3),
    "short_baseline": (dict(seed=14, kind="short"), 4),
    "identical": (dict(seed=15, kind="identical"), 5),
    "forward_similar": (dict(seed=16, kind="forward"), 6),
    "plane_tilted": (dict(seed=21, kind="plane", tilt=0.8, baseline=1.2), 7),
    "low_parallax_f": (dict(seed=22, kind="general", baseline=0.08), 8),
    "few_points": (dict(seed=21, kind="plane", tilt=0.8, baseline=1.2, N=45), 9),
    "noisy_plane": (dict(seed=22, kind="plane", tilt=0.8, baseline=1.2, noise=1.2), 9),
}
# what each named scene must be followed to by compare(), on the library's own selection: (model, success, reason bits that must be set)
NAMED_EXIT = {"general": (2, True, 0), "plane": (1, False, H_SECOND), "outliers40": (2, False, F_FEW_GOOD),
              "short_baseline": (1, False, H_PARALLAX), "identical": (1, False, H_DEGENERATE), "forward_similar": (1, False, H_SECOND),
              "plane_tilted": (1, True, 0), "low_parallax_f": (2, False, F_PARALLAX), "few_points": (1, False, H_MIN_TRIANGULATED),
              "noisy_plane": (2, False, F_SIMILAR)}


def assert_followed_to_its_exit(name, out):
    """after compare(name, out): the reconstruction half ran on the library's selection, its acceptance was a parity decision (so
    success and reason WERE compared with the float64 reading), and the scene took the exit it is named for"""
    info, (model, success, bits) = compare.last, NAMED_EXIT[name]
    assert info["reconstructed"] and info["decide_parity"], (name, info)
    assert info["candidates"] == (0 if name == "identical" else (8 if model == 1 else 4)), (name, info)
    assert int(out["result"]["model"]) == model and bool(out["result"]["success"]) == success == info["success64"], (name, info)
    assert int(out["result"]["reason"]) & bits == bits == info["reason64"] & bits, (name, info)
    assert (info["points"] > 50) == success, (name, info)


# what the directed scenes must reach between them (census); see the module docstring for what no scene reaches
EXPECTED_CENSUS = {"success_f", "success_h", "h_degenerate", "f_few_good", "f_similar", "f_parallax", "h_second", "h_parallax",
                   "h_min_triangulated", "rt_behind1", "rt_behind2", "rt_reproj1", "rt_reproj2", "rt_good_low_parallax", "rt_good"}
H_ACCURACY = 64


def draw_sets(N, H, seed):
    """the swap-with-back sampling of :80-93 on a numpy Generator"""
    rng = np.random.default_rng(seed)
    out = np.empty((H, 8), np.int32)
    for h in range(H):
        avail = list(range(N))
        for j in range(8):
            k = int(rng.integers(len(avail)))
            out[h, j] = avail[k]
            avail[k] = avail[-1]
            avail.pop()
    return out


def build_case(name):
    args, set_seed = CASES[name]
    keys1, keys2, m12, params, truth = scene(**args)
    sets = draw_sets(int((m12 >= 0).sum()), H_ACCURACY, set_seed)
    return {"name": name, "keys1": keys1, "keys2": keys2, "matches12": m12, "sets": sets, "params": params, "truth": truth}


_cache = {}


def solved(name):
    """the case with its R64 and R32 runs and verdicts, computed once"""
    if name not in _cache:
        c = build_case(name)
        c["r64"] = run(c["keys1"], c["keys2"], c["matches12"], c["sets"], c["params"], "R64")
        c["r32"] = run(c["keys1"], c["keys2"], c["matches12"], c["sets"], c["params"], "R32")
        c["v"] = verdicts(c["r64"], c["r32"])
        _cache[name] = c
    return _cache[name]


# ---- the comparison the CPU suite applies to the host build and the GPU suite to the device
def _sign_to(a, ref):
    return a * np.where((a * ref).sum(-1, keepdims=True) < 0, -1.0, 1.0)


def _rule(e_got, e_32, label, rows, name):
    ulp = 2.0 ** -23
    if not len(e_got):
        return
    med, mx = (np.median(e_got), np.median(e_32)), (e_got.max(), e_32.max())
    rows.append((name, label, len(e_got), med[1], mx[1], med[0], mx[0]))
    print(f"{name}: {label} ({len(e_got)}): e(R32) median {med[1]:.3g} max {mx[1]:.3g}; e(got) median {med[0]:.3g} max {mx[0]:.3g}")
    assert med[0] <= 4 * med[1] + 2 * ulp and mx[0] <= 4 * mx[1] + 2 * ulp, (name, label)


def compare(name, out, rows=None):
    """`out`: what initializer.initialize returns with every optional output, for case `name`.  Asserts the criteria of the module
    docstring and the error rule median e(got) <= 4 median e(R32) + 2 ulp (and the same for the maximum) against R64, every error
    relative to the magnitude of what it measures; appends (case, quantity, n, e32 median, e32 max, got median, got max) to rows."""
    c = solved(name)
    r64, r32, v = c["r64"], c["r32"], c["v"]
    rows = [] if rows is None else rows
    res = out["result"]
    N = r64["N"]
    assert int(res["n_matches"]) == N
    # Normalize: bit-equal to the float32 reading
    assert np.array_equal(np.asarray(res["norm1"], F32).view(np.uint32), r32["norm1"].astype(F32).view(np.uint32)), name
    assert np.array_equal(np.asarray(res["norm2"], F32).view(np.uint32), r32["norm2"].astype(F32).view(np.uint32)), name
    for key, T in (("norm1", r32["T1"]), ("norm2", r32["T2"])):   # T1 / T2 rebuilt from the record: -mean * s in float, as :780-781
        mx, my, sx, sy = (F32(x) for x in res[key])
        Tgot = np.array([[sx, 0, F32(-mx) * sx], [0, sy, F32(-my) * sy], [0, 0, 1]], F32)
        assert np.array_equal(Tgot.view(np.uint32), T.astype(F32).view(np.uint32)), (name, key)
    got_scores = {}
    for k in ("h", "f"):
        hyps, words = out["hyps_" + k], out["words_" + k]
        b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(len(words), -1), axis=1, bitorder="little").astype(bool)
        assert not b[:, N:].any(), "tail bits are zero"
        b = b[:, :N]
        assert np.array_equal(hyps["status"] == 1, r64["ok"])
        assert np.array_equal(hyps["n_inliers"], b.sum(1)), "the count is the popcount of the word row"
        par = v["inl_" + k]
        assert np.array_equal(b[par], r32["inl_" + k][par]), f"{name}: {k} inlier bits differ from the reading on parity decisions"
        sc = hyps["score"]
        got_scores[k] = sc
        # the selection rule over the device's OWN scores, exactly
        want = first_max(sc)
        assert int(res["best_" + k]) == want, (name, k)
        assert res["score_" + k] == (sc[want] if want >= 0 else 0)
        if v["win_" + k]:
            assert want == r64["best_" + k], (name, k)
        # matrices of hypotheses with a null-space gap, up to sign and scale 1 (unit null vector): relative to the Frobenius norm
        hp = v["hyp_" + k]
        ref = r64[("H21" if k == "h" else "F21")][hp].reshape(-1, 9)
        nrm = np.linalg.norm(ref, axis=1, keepdims=True)
        eg = np.abs(_sign_to(hyps["M"][hp].astype(F64), ref) - ref) / nrm
        e32 = np.abs(_sign_to(r32[("H21" if k == "h" else "F21")][hp].reshape(-1, 9).astype(F64), ref) - ref) / nrm
        _rule(eg.max(1), e32.max(1), "H21" if k == "h" else "F21", rows, name)
        # scores of hypotheses whose inlier decisions are all parity
        full = par.all(1) & r64["ok"] & (r64["score_" + k] > 0)
        _rule(np.abs(sc[full] - r64["score_" + k][full]) / r64["score_" + k][full],
              np.abs(r32["score_" + k][full].astype(F64) - r64["score_" + k][full]) / r64["score_" + k][full], "score_" + k, rows, name)
    if v["model"]:
        assert int(res["model"]) == r64["model"], name
    # The reconstruction half.  Its input is a selection: the model, the winner's matrix and its inlier verdicts.  Where the
    # yardstick's own selection is a parity decision the library's must be the same one (asserted above); in every case the
    # yardstick's reconstruction stages are run in float64 and in float32 on the selection the LIBRARY made -- its float matrix, its
    # verdicts -- so that candidates, CheckRT, the acceptance rules and the outputs are compared with an independent reading also where
    # another hypothesis won by a hair.
    info = {"reconstructed": False, "decide_parity": False, "candidates": 0, "points": 0}
    model = int(res["model"])
    assert model in (1, 2) or (r64["model"] == 0 and int(res["n_candidates"]) == 0), name
    if model in (1, 2):
        Msel = np.asarray(res["H21" if model == 1 else "F21"], F32)
        bsel = int(res["best_h" if model == 1 else "best_f"])
        assert np.array_equal(Msel, out["hyps_" + ("h" if model == 1 else "f")]["M"][bsel])
        sel_inl = np.asarray(out["inliers"], bool)
        bits_sel = np.unpackbits(np.ascontiguousarray(out["words_" + ("h" if model == 1 else "f")][bsel]).view(np.uint8), bitorder="little")
        assert np.array_equal(sel_inl, bits_sel[:N].astype(bool)) and int(res["n_inliers"]) == int(sel_inl.sum())
        n1 = len(out["P3D"])
        a64 = reconstruct(model, Msel.astype(F64), sel_inl, r64["m"], r64["K"], r64["i1"], n1, c["params"], F64)
        a32 = reconstruct(model, Msel, sel_inl, r64["m"], r64["K"], r64["i1"], n1, c["params"], F32)
        w = rt_verdicts(a64, a32)
        info.update(reconstructed=True, decide_parity=w["decide"], reason64=a64["reason"], success64=a64["success"])
        assert int(res["n_candidates"]) == len(a64["cands"]), name
        if w["decide"]:
            assert (int(res["success"]), int(res["reason"]) & w["mask"]) == (int(a64["success"]), a64["reason"] & w["mask"]), name
        if a64["cands"] and w["rt"]:
            got = [{"R": out["candidates"]["R"][j].reshape(3, 3), "t": out["candidates"]["t"][j]} for j in range(len(a64["cands"]))]
            order = match_candidates(a64["cands"], got)
            o32 = match_candidates(a64["cands"], a32["cands"])
            info["candidates"] = len(order)
            eR, eR32, et, et32, ep, ep32 = [], [], [], [], [], []
            for i, (cr, j, j32) in enumerate(zip(a64["cands"], order, o32)):
                eR.append(np.abs(got[j]["R"] - cr["R"]).max()); eR32.append(np.abs(a32["cands"][j32]["R"].astype(F64) - cr["R"]).max())
                et.append(np.abs(got[j]["t"] - cr["t"]).max()); et32.append(np.abs(a32["cands"][j32]["t"].astype(F64) - cr["t"]).max())
                loose = int((~w["rt"][i]).sum())
                g = int(out["candidates"]["n_good"][j])
                lo = int(((cr["code"] >= 5) & w["rt"][i]).sum())
                assert lo <= g <= lo + loose, f"{name}: candidate {i}: n_good {g} leaves the room [{lo}, {lo + loose}] of the parity decisions"
                if cr["n_good"] > 51 + loose and cr["parallax"] > 0:   # the order statistic is the 51st: a count change does not move it
                    # measured where the float rounding happens, on the cosine (magnitude 1): acos near 1 turns one ulp of it into
                    # ulp / sin(parallax) radians, which no reading in float can avoid
                    cosd = lambda x: np.cos(np.deg2rad(F64(x)))
                    ep.append(abs(cosd(out["candidates"]["parallax"][j]) - cosd(cr["parallax"])))
                    ep32.append(abs(cosd(a32["cands"][j32]["parallax"]) - cosd(cr["parallax"])))
            _rule(np.array(eR), np.array(eR32), "R", rows, name)
            _rule(np.array(et), np.array(et32), "t", rows, name)
            _rule(np.array(ep), np.array(ep32), "cos(parallax)", rows, name)
            if w["decide"]:   # which candidate wins, its count and the runner-up figure
                lo_hi = sum(int((~x).sum()) for x in w["rt"])
                g64 = sorted((cr["n_good"] for cr in a64["cands"]), reverse=True)
                if a64["best_candidate"] < 0:
                    assert int(res["best_candidate"]) == -1, name
                elif g64[0] - g64[1] > lo_hi:   # a unique best; among equal counts the first wins, and the ORDER of the candidates is free
                    assert order[a64["best_candidate"]] == int(res["best_candidate"]), name
                assert abs(int(res["n_good"]) - a64["n_good"]) <= lo_hi, name
        if w["decide"] and a64["success"]:
            bc64 = a64["best_candidate"]
            par = np.ones(n1, bool)
            par[r64["i1"]] = w["rt"][bc64]
            assert np.array_equal(out["triangulated"][par], a64["triangulated"][par]), name
            set64 = (a64["P3D"] != 0).any(1)
            assert np.array_equal((out["P3D"] != 0).any(1)[par], set64[par]), name
            both = par & set64
            info["points"] = int(both.sum())
            nrm = np.linalg.norm(a64["P3D"][both], axis=1)
            _rule(np.abs(out["P3D"][both] - a64["P3D"][both]).max(1) / nrm, np.abs(a32["P3D"][both].astype(F64) - a64["P3D"][both]).max(1) / nrm,
                  "P3D", rows, name)
            assert int(res["n_triangulated"]) == int(out["triangulated"].sum())
            bc = int(res["best_candidate"])   # R21 / t21 are the winning candidate's own bits
            assert np.array_equal(res["R21"], out["candidates"]["R"][bc]) and np.array_equal(res["t21"], out["candidates"]["t"][bc])
        elif not int(res["success"]):
            assert not out["P3D"].any() and not out["triangulated"].any() and not np.asarray(res["R21"]).any(), name
    compare.last = info
    return rows
