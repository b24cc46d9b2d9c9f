"""GPU: orbfe_optimize_sim3 / orbfe_optimize_sim3_batch_device (Optimizer::OptimizeSim3 on the device) against the numpy reading of
tests/np_optsim3.py -- never against itself or against csrc/optsim3_internal.h compiled for the host.

Criterion (derived, not tuned): the scale within 2^-23 * s, every rotation entry within 2^-23, every translation entry within
2^-23 * max(1, |t|_inf) -- one unit in the last place of a float at the scale of the block, both sides computing in double and
rounding once; the bad flags, n_pairs, n_bad and n_inliers EQUAL; iterations reported only.  Every figure is printed before it is
asserted."""
import ctypes as C

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from refactored_orb_slam2_amd._lib import OPTSIM3_PAIR_DTYPE, OPTSIM3_RESULT_DTYPE, SIM3_VIEW_DTYPE
from tests import np_optsim3 as Q

pytestmark = pytest.mark.gpu


def _view(v):
    return optimizer.sim3_view(v["Rcw"], v["tcw"], v["fx"], v["fy"], v["cx"], v["cy"])


def _sRt(res):
    return np.concatenate([[res["s"]], res["R"], res["t"]]).astype(np.float32)


def _compare(name, res, bad, ref):
    """prints the figures, then asserts the criterion"""
    v, vr = _sRt(res), ref["sRt"]
    d = np.abs(v.astype(np.float64) - vr.astype(np.float64))
    tol = Q.tolerance(vr)
    not_equal = int((v.view(np.uint32) != vr.view(np.uint32)).sum())
    flags_differ = int((np.asarray(bad) != ref["bad"]).sum())
    print(f"optsim3 parity {name}: max diff / tolerance {float((d / tol).max()):.3f}, entries not bit-equal {not_equal}/13, flags that "
          f"differ {flags_differ}, n_pairs {int(res['n_pairs'])}/{ref['n_pairs']}, n_bad {int(res['n_bad'])}/{ref['n_bad']}, n_inliers "
          f"{int(res['n_inliers'])}/{ref['n_inliers']}, iterations {list(res['iterations'])} (reading {ref['iterations']})")
    assert flags_differ == 0, name
    assert (int(res["n_pairs"]), int(res["n_bad"]), int(res["n_inliers"])) == (ref["n_pairs"], ref["n_bad"], ref["n_inliers"]), name
    assert np.all(d <= tol), (name, d / tol)


def _host(s):
    return optimizer.optimize_sim3(_view(s["view1"]), _view(s["view2"]), s["pairs"], s["sRt_in"], s["th2"], s["fix_scale"])


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a).cuda()


class Batch:
    """Scenes stacked into one batch: ragged counts, the padding rows of `cap` filled with garbage, d_bad with sentinel bytes"""

    def __init__(self, scenes, pad=13):
        import torch
        self.scenes, B = scenes, len(scenes)
        self.cap = max(len(s["pairs"]) for s in scenes) + pad
        rng = np.random.default_rng(7)
        pairs = rng.integers(0, 256, (B, self.cap, OPTSIM3_PAIR_DTYPE.itemsize), dtype=np.uint8).view(OPTSIM3_PAIR_DTYPE).reshape(B, self.cap)
        v1, v2 = np.zeros(B, SIM3_VIEW_DTYPE), np.zeros(B, SIM3_VIEW_DTYPE)
        n, sRt, th2, fix = np.zeros(B, np.int32), np.zeros((B, 13), np.float32), np.zeros(B, np.float32), np.zeros(B, np.int32)
        for p, s in enumerate(scenes):
            m = len(s["pairs"])
            pairs[p, :m], n[p], sRt[p], th2[p], fix[p] = s["pairs"], m, s["sRt_in"], s["th2"], 7 if s["fix_scale"] else 0
            v1[p], v2[p] = _view(s["view1"])[0], _view(s["view2"])[0]
        self.t = [_dev(x) for x in (v1, v2, pairs, n, sRt, th2, fix)]
        self.res = torch.zeros((B, OPTSIM3_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        self.bad = torch.full((B, self.cap), 0xEE, dtype=torch.uint8, device="cuda")

    def run(self):
        import torch
        st = torch.cuda.Stream()
        optimizer.optimize_sim3_batch(*self.t, self.res, self.bad, stream=st)
        st.synchronize()
        return self.res.cpu().numpy().view(OPTSIM3_RESULT_DTYPE).reshape(-1), self.bad.cpu().numpy()


@pytest.fixture(scope="module")
def refs():
    return {name: (Q.case_scene(name), Q.run_case(Q.case_scene(name))) for name in Q.CASES}


@pytest.mark.parametrize("name", list(Q.CASES))
def test_host_form_against_the_reading(refs, name):
    """includes the case larger than the LDS cache (2 100 pairs against 2 048 cached rows), n == 9 and n == 0"""
    s, ref = refs[name]
    res, bad = _host(s)
    _compare(name, res, bad, ref)
    if ref["n_inliers"] == 0:   # returned 0: the transform is the input bit for bit, the flags are written all the same
        assert np.array_equal(_sRt(res).view(np.uint32), s["sRt_in"].view(np.uint32)), name
        assert int(res["iterations"][1]) == 0
        if name.startswith("pairs_12") or name == "pairs_9":
            assert bad.sum() == ref["n_bad"] > 0


def test_batch_form_against_the_reading(refs):
    """every case in batches of at most 12: ragged counts (0 .. 2 100), fixed and free scale and two values of th2 mixed, garbage in
    the padding rows, rows behind d_n[p] untouched"""
    names = list(Q.CASES)
    for group in (names[:12], names[12:] + ["th2_7", "free_scale", "pairs_0"]):
        assert len({float(refs[n][0]["th2"]) for n in group}) > 1 and len({refs[n][0]["fix_scale"] for n in group}) == 2
        b = Batch([refs[n][0] for n in group])
        res, bad = b.run()
        for p, name in enumerate(group):
            m = len(refs[name][0]["pairs"])
            _compare(f"batch:{name}", res[p], bad[p, :m], refs[name][1])
            assert np.all(bad[p, m:] == 0xEE), "rows behind d_n[p] must not be written"


def test_a_problem_does_not_depend_on_the_batch(refs):
    """result and flags byte-identical: the host form, alone in a batch, at every position of a batch of three, in a batch of five,
    and in a second run"""
    for name in ("free_scale", "survivors_10", "beyond_cache"):
        s = refs[name][0]
        m = len(s["pairs"])
        res0, bad0 = _host(s)
        want = (res0.tobytes(), bad0.tobytes())
        others = [refs["pairs_24"][0], refs["outliers_40"][0], refs["clean"][0], refs["pairs_9"][0]]
        layouts = [[s], [s, others[0], others[1]], [others[0], s, others[1]], [others[0], others[1], s], [others[2], others[3], s, others[0], s],
                   [s]]
        for k, scenes in enumerate(layouts):
            res, bad = Batch(scenes, pad=k).run()
            for p, sc in enumerate(scenes):
                if sc is s:
                    assert (res[p].tobytes(), bad[p, :m].tobytes()) == want, (name, k, p)
        print(f"determinism {name}: {sum(sc is s for l in layouts for sc in l)} placements byte-identical to the host form")


def test_counts_are_clamped_and_empty_batches_launch_nothing(refs):
    import torch
    s = refs["pairs_24"][0]
    b = Batch([s, s], pad=0)
    res_ref, bad_ref = b.run()
    b.t[3] = _dev(np.array([b.cap + 1000, -5], np.int32))   # clamped to [0, cap]: problem 0 unchanged, problem 1 empty
    b.bad.fill_(0xEE)
    res, bad = b.run()
    assert res[0].tobytes() == res_ref[0].tobytes() and np.array_equal(bad[0], bad_ref[0])
    assert int(res[1]["n_pairs"]) == 0 and int(res[1]["n_inliers"]) == 0 and np.all(bad[1] == 0xEE)
    assert np.array_equal(_sRt(res[1]).view(np.uint32), s["sRt_in"].view(np.uint32))
    L = _lib.lib()
    p = [_lib.ptr(x) for x in b.t]
    assert L.orbfe_optimize_sim3_batch_device(0, p[0], p[1], p[2], p[3], b.cap, p[4], p[5], p[6], _lib.ptr(b.res), _lib.ptr(b.bad), None) == _lib.OK
    torch.cuda.synchronize()


def test_validation_with_a_device(refs):
    """every limit at its boundary, with a device present: the largest accepted value runs, the first refused one is ORBFE_ERR_INVALID"""
    L = _lib.lib()
    s = refs["pairs_24"][0]
    v1, v2 = _view(s["view1"]), _view(s["view2"])
    res = np.zeros(1, OPTSIM3_RESULT_DTYPE)
    big = np.zeros(_lib.OPTSIM3_MAX_PAIRS + 1, OPTSIM3_PAIR_DTYPE)
    big[:] = s["pairs"][0]
    bad = np.zeros(len(big), np.uint8)
    call = lambda n, th2: L.orbfe_optimize_sim3(_lib.ptr(v1), _lib.ptr(v2), _lib.ptr(big), n, _lib.ptr(s["sRt_in"]), C.c_float(th2), 1,
                                                _lib.ptr(res), _lib.ptr(bad))
    assert call(_lib.OPTSIM3_MAX_PAIRS, 10.0) == _lib.OK and int(res[0]["n_pairs"]) == _lib.OPTSIM3_MAX_PAIRS
    assert call(_lib.OPTSIM3_MAX_PAIRS + 1, 10.0) == _lib.ERR_INVALID
    assert call(-1, 10.0) == _lib.ERR_INVALID
    assert call(24, 0.0) == _lib.ERR_INVALID and call(24, float("nan")) == _lib.ERR_INVALID
    assert call(24, float(np.nextafter(np.float32(0), np.float32(1)))) == _lib.OK
    b = Batch([s], pad=0)
    p = [_lib.ptr(x) for x in b.t]
    batch = lambda P, cap: L.orbfe_optimize_sim3_batch_device(P, p[0], p[1], p[2], p[3], cap, p[4], p[5], p[6], _lib.ptr(b.res),
                                                              _lib.ptr(b.bad), None)
    assert batch(-1, b.cap) == _lib.ERR_INVALID and batch(_lib.OPTSIM3_MAX_PROBLEMS + 1, b.cap) == _lib.ERR_INVALID
    assert batch(1, -1) == _lib.ERR_INVALID and batch(1, _lib.OPTSIM3_MAX_PAIRS + 1) == _lib.ERR_INVALID
    assert batch(1, b.cap) == _lib.OK
    import torch
    torch.cuda.synchronize()


# ---- end to end: Sim3Solver -> SearchBySim3 -> OptimizeSim3 -----------------------------------------------------------------------
def _chain_scene(seed, n=160, n_levels=8):
    """Two keyframes for the three steps of LoopClosing::ComputeSim3 behind SearchByBoW: the scene of np_optsim3.make_scene (free scale,
    15 % of the observations displaced by 4 - 40 px) with one keypoint per point in either keyframe (keyframe 2's permuted), the same
    octave on both sides, a random 256-bit descriptor per point with 6 bits flipped in keyframe 2, scale-invariance distances as
    MapPoint::UpdateNormalAndDepth sets them from the point's own observation, and keyframe 2's map points displaced by N(0, 1e-3 x
    depth) per axis (0.7 px): without it the solver, which sees the points only, would return the true similarity."""
    from refactored_orb_slam2_amd._lib import KF_CAMERA_DTYPE, KF_POINT_DTYPE, KP_DTYPE
    s = Q.make_scene(seed, n_pairs=n, outliers=0.15, fix_scale=False, true_scale=1.05, n_levels=n_levels)
    rng = np.random.default_rng(seed + 500)
    depth2 = Q.camera_points(s["view2"], s["pairs"]["Xw2"])[:, 2].astype(np.float64)
    s["pairs"]["Xw2"] = (s["pairs"]["Xw2"].astype(np.float64) + rng.normal(size=(n, 3)) * (1e-3 * depth2)[:, None]).astype(np.float32)
    sf = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        sf[i] = sf[i - 1] * np.float32(1.2)
    octv = s["oct1"]
    perm2 = rng.permutation(n)                                              # keypoint of point i in keyframe 2
    desc1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc2 = desc1.copy()
    for i in range(n):
        for b in rng.choice(256, 6, replace=False):
            desc2[i, b >> 3] ^= np.uint8(1 << (b & 7))
    kf = []
    for obs, idx, desc in ((s["pairs"]["obs1"], np.arange(n), desc1), (s["pairs"]["obs2"], perm2, desc2)):
        k = np.zeros(n, KP_DTYPE)
        k["x"][idx], k["y"][idx], k["octave"][idx] = obs[:, 0], obs[:, 1], octv
        k["size"], k["angle"], k["class_id"] = 31.0, 10.0, -1
        d = np.zeros((n, 32), np.uint8)
        d[idx] = desc
        kf.append((k, d))
    pts = []
    for view, Xw, desc in ((s["view1"], s["pairs"]["Xw1"], desc1), (s["view2"], s["pairs"]["Xw2"], desc2)):
        p = np.zeros(n, KF_POINT_DTYPE)
        dist = np.linalg.norm(Q.camera_points(view, Xw).astype(np.float64), axis=1)
        p["pos"], p["desc"], p["angle"] = Xw, desc, 10.0
        p["max_distance"] = (dist * sf[octv]).astype(np.float32)             # mfMaxDistance, mfMinDistance (MapPoint.cc:371-374)
        p["min_distance"] = (dist * sf[octv] / sf[-1]).astype(np.float32)
        pts.append(p)

    def camera(view_from, view_to, sR, t):
        c = np.zeros(1, KF_CAMERA_DTYPE)
        c["R"], c["t"], c["R2"], c["t2"] = view_from["Rcw"], view_from["tcw"], np.asarray(sR, np.float32).reshape(9), np.asarray(t, np.float32)
        for f in ("fx", "fy", "cx", "cy"):
            c[f] = view_to[f]
        c["min_x"], c["max_x"], c["min_y"], c["max_y"] = 0, 1241, 0, 376
        c["log_scale_factor"], c["n_levels"], c["th"] = np.float32(np.log(np.float32(1.2))), n_levels, 7.5
        c["scale_factors"][0, :n_levels] = sf
        return c

    return dict(s=s, sf=sf, octv=octv, perm2=perm2, kf=kf, pts=pts, camera=camera, n=n, inv_sigma2=s["inv_level_sigma2"])


def _search_by_sim3(c, sRt, search):
    """ORBmatcher::SearchBySim3 (L/src/ORBmatcher.cc:1029-1245) on two one-direction searches: `search(direction, camera, points)`
    returns best_idx per point; the matches are those the two directions agree on (:1225-1242).  Returns (i1, j2) index arrays."""
    s12, R12, t12 = np.float32(sRt[0]), np.asarray(sRt[1:10], np.float32).reshape(3, 3), np.asarray(sRt[10:13], np.float32)
    sR12 = s12 * R12                                                        # :1044-1047 in float
    sR21 = (np.float32(1.0) / s12) * R12.T
    t21 = -(sR21 @ t12)
    v1, v2 = c["s"]["view1"], c["s"]["view2"]
    a = search(0, c["camera"](v1, v2, sR21, t21), c["pts"][0])                # keyframe 1's points into keyframe 2
    b = search(1, c["camera"](v2, v1, sR12, t12), c["pts"][1])                # keyframe 2's points into keyframe 1
    match2_of_kp1 = a                                                       # point i of keyframe 1 is its keypoint i
    match1_of_kp2 = np.full(c["n"], -1, np.int64)
    match1_of_kp2[c["perm2"]] = b                                           # point i of keyframe 2 is its keypoint perm2[i]
    i1 = np.array([i for i in range(c["n"]) if match2_of_kp1[i] >= 0 and match1_of_kp2[match2_of_kp1[i]] == i], np.int64)
    return i1, match2_of_kp1[i1].astype(np.int64)


def _optsim3_pairs(c, i1, j2):
    inv2 = np.argsort(c["perm2"])                                           # keypoint of keyframe 2 -> its point
    p = np.zeros(len(i1), OPTSIM3_PAIR_DTYPE)
    p["Xw1"], p["Xw2"] = c["pts"][0]["pos"][i1], c["pts"][1]["pos"][inv2[j2]]
    k1, k2 = c["kf"][0][0], c["kf"][1][0]
    p["obs1"] = np.stack([k1["x"][i1], k1["y"][i1]], 1)
    p["obs2"] = np.stack([k2["x"][j2], k2["y"][j2]], 1)
    p["inv_sigma2_1"], p["inv_sigma2_2"] = c["inv_sigma2"][k1["octave"][i1]], c["inv_sigma2"][k2["octave"][j2]]
    return p


@pytest.mark.parametrize("seed", [21, 22])
def test_chain_solver_search_optimizer_against_the_readings(seed):
    """orbfe_sim3_solve_batch_device -> orbfe_kf_search (ORBFE_KF_SIM3, both directions) -> orbfe_optimize_sim3_batch_device on
    synthetic two-keyframe data against the same three steps done with the readings (tests/np_sim3.py, the oracle's SearchBySim3,
    tests/np_optsim3.py), each chain feeding on its own results"""
    import torch
    from refactored_orb_slam2_amd import sim3
    from refactored_orb_slam2_amd.matcher import FrameView, ORBmatcher
    from tests import np_sim3 as S
    from tests import oracle_lib as ol
    c = _chain_scene(seed)
    s, n, H, MIN = c["s"], c["n"], 48, 20
    v1, v2 = _view(s["view1"]), _view(s["view2"])
    # step 1 on the first 100 correspondences (what SearchByBoW would have handed over)
    m = 100
    sig2 = (c["sf"] * c["sf"])[c["octv"][:m]]
    sp = sim3.sim3_pairs(s["pairs"]["Xw1"][:m], s["pairs"]["Xw2"][:m], sim3.max_error(sig2), sim3.max_error(sig2))
    tr = sim3.draw_triples(m, H, np.random.default_rng(seed))
    W = (m + 63) // 64
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device="cuda")
    i32 = lambda x: _dev(np.array([x], np.int32))
    d_res = z(1, 128)
    st = torch.cuda.Stream()
    sim3.sim3_solve_batch(_dev(v1), _dev(v2), _dev(sp).view(1, m, 32), i32(m), _dev(tr).view(1, H, 3), i32(H), i32(0), i32(MIN), z(1, H, 64),
                          z(1, H, W, dt=torch.int64), d_res, z(1, W, dt=torch.int64), stream=st)
    st.synchronize()
    r1 = d_res.cpu().numpy().view(_lib.SIM3_RESULT_DTYPE).reshape(-1)[0]
    ref1 = S.solve(v1, v2, sp, tr, False, mode="R64")
    ret_ref, _ = S.select(ref1["count"], MIN)
    print(f"chain {seed}: solver returned hypothesis {int(r1['returned'])} (reading {ret_ref}) with {int(r1['n_inliers'])} inliers "
          f"(reading {int(ref1['count'][ret_ref])})")
    # the conditions of a parity case, on the reading: a hypothesis is returned, and no count up to it sits at the acceptance rule
    assert ret_ref >= 0 and not np.any(np.abs(ref1["count"][:ret_ref + 1].astype(np.int64) - MIN) <= 1)
    assert int(r1["returned"]) == ret_ref
    sRt_dev = np.concatenate([[r1["s"]], r1["R"], r1["t"]]).astype(np.float32)
    sRt_ref = np.concatenate([[ref1["s"][ret_ref]], ref1["R"][ret_ref].reshape(9), ref1["t"][ret_ref]]).astype(np.float32)
    # step 2
    mt = ORBmatcher(0.8, True)
    frames = [FrameView(k, d, 0, 1241, 0, 376) for k, d in c["kf"]]
    oframes = [ol.OracleFrame(k, d, c["sf"], 0, 1241, 0, 376) for k, d in c["kf"]]
    dev_search = lambda direction, cam, pts: mt.KeyFrameSearch(frames[1 - direction], cam, pts, _lib.KF_SIM3)[1]["best_idx"]
    ref_search = lambda direction, cam, pts: ol.kf_search(oframes[1 - direction], cam, pts, 3)[1]["best_idx"]
    i1, j2 = _search_by_sim3(c, sRt_dev, dev_search)
    i1r, j2r = _search_by_sim3(c, sRt_ref, ref_search)
    print(f"chain {seed}: SearchBySim3 kept {len(i1)} of {n} (readings {len(i1r)}), {int((c['perm2'][i1] == j2).sum())} of them true pairs")
    assert np.array_equal(i1, i1r) and np.array_equal(j2, j2r) and len(i1) >= 100
    # step 3
    pairs, pairs_r = _optsim3_pairs(c, i1, j2), _optsim3_pairs(c, i1r, j2r)
    ref3 = Q.optimize_sim3(s["view1"], s["view2"], pairs_r, sRt_ref, 10.0, False)
    margin = Q.min_margin(ref3, 10.0)
    print(f"chain {seed}: margin of the reading {margin:.3g}")
    assert margin >= 1e-4
    b = Batch([dict(view1=s["view1"], view2=s["view2"], pairs=pairs, sRt_in=sRt_dev, th2=np.float32(10.0), fix_scale=False)])
    res, bad = b.run()
    _compare(f"chain {seed}", res[0], bad[0, :len(pairs)], ref3)
    assert int(res[0]["n_inliers"]) >= 20                                   # LoopClosing.cc:316: the candidate is accepted
    e_in = np.abs(sRt_dev.astype(np.float64) - s["sRt_true"]).max()
    e_out = np.abs(_sRt(res[0]).astype(np.float64) - s["sRt_true"]).max()
    print(f"chain {seed}: error of the similarity {e_in:.3g} -> {e_out:.3g}")
