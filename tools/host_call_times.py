#!/usr/bin/env python3
"""Host-clock latency of the one-problem host entry points that no other tool times: pose optimisation, triangulation, the Sim3
solver, OptimizeSim3, local bundle adjustment and the map-point refresh on the standard scenes of their suites (tests/np_*.py), and
the matcher forms SearchByBoW (frame and keyframe), proj_best, kf_search (Fuse and the loop search), SearchLocalPoints and
SearchForInitialization on one extracted 1241 x 376 frame pair.  Each form is called through its Python wrapper (the wrapper's own
cost is part of every figure, the same for every library), warm, N times; one JSON line with the median and the 10th percentile in
milliseconds per form.  A/B builds: ORBFE_AB_LIB=<name> (refactored_orb_slam2_amd/csrc/_ab/liborbfe_<name>.so).

usage: python tools/host_call_times.py [--reps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refactored_orb_slam2_amd import _lib  # noqa: E402
if os.environ.get("ORBFE_AB_LIB"): _lib.LIB_PATH = os.path.join(_lib.CSRC, "_ab", "liborbfe_%s.so" % os.environ["ORBFE_AB_LIB"])
from refactored_orb_slam2_amd import ORBextractor, map_point, mapping, optimizer, sim3, synth  # noqa: E402
from refactored_orb_slam2_amd.matcher import FrameView, ORBmatcher, make_frustum, make_queries, search_by_bow_kf  # noqa: E402


def _case(mod):
    return mod.case_scene("standard" if "standard" in mod.CASES else list(mod.CASES)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from tests import np_lba, np_mapping, np_mappoint, np_optsim3, np_pose, np_sim3
    forms = {}

    s = _case(np_pose)
    keys = np.zeros(len(s["keys_xy"]), _lib.KP_DTYPE)
    keys["x"], keys["y"], keys["octave"] = s["keys_xy"][:, 0], s["keys_xy"][:, 1], s["octave"]
    c = s["cam"]
    cam = optimizer.pose_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], c["inv_level_sigma2"])
    forms["pose_optimization"] = lambda: optimizer.pose_optimization(keys, s["u_right"], s["assigned"], s["points"], cam, s["Tcw_in"])

    t = np_mapping.scene_args(_case(np_mapping))
    forms["triangulate_matches"] = lambda: mapping.triangulate_matches(*t)

    s3 = _case(np_sim3)
    forms["sim3_solve"] = lambda: sim3.sim3_solve(s3["view1"], s3["view2"], s3["pairs"], s3["triples"], s3["fix_scale"], s3["min_inliers"])

    so = _case(np_optsim3)
    view = lambda v: optimizer.sim3_view(v["Rcw"], v["tcw"], v["fx"], v["fy"], v["cx"], v["cy"])
    v1, v2 = view(so["view1"]), view(so["view2"])
    forms["optimize_sim3"] = lambda: optimizer.optimize_sim3(v1, v2, so["pairs"], so["sRt_in"], so["th2"], so["fix_scale"])

    sl = _case(np_lba)
    cl = sl["cam"]
    lcam = optimizer.pose_camera(cl["fx"], cl["fy"], cl["cx"], cl["cy"], cl["mbf"], [1.0])
    forms["local_bundle_adjustment"] = lambda: optimizer.local_bundle_adjustment(lcam, sl["poses"], sl["fixed"], sl["points"], sl["edges"])

    sm = np_mappoint.make_scene(101, [1, 2, 3, 5, 8, 13, 21, 40, 63, 64, 65, 80, 100] * 8)
    forms["refresh_map_points"] = lambda: map_point.refresh_map_points(sm["keyframes"], sm["points"], sm["scale_factors"])

    # ---- the matcher forms on one extracted frame pair
    w, h = 1241, 376
    a, b = synth.sequence(w, h, 2, seq=9)[:2]
    ex = ORBextractor(2000, device=0)
    k0, d0 = ex(a); k1, d1 = ex(b)
    sf = ex.GetScaleFactors(); inv_s2 = ex.GetInverseScaleSigmaSquares()
    ex.close()
    rng = np.random.default_rng(3)
    ur = np.where(rng.random(len(k1)) < 0.5, k1["x"] - np.float32(20.0), np.float32(-1)).astype(np.float32)
    fv, fv_mono, f0 = FrameView(k1, d1, 0, w, 0, h, ur), FrameView(k1, d1, 0, w, 0, h), FrameView(k0, d0, 0, w, 0, h)
    q = make_queries(len(k0))
    q["u"], q["v"], q["u_r"] = k0["x"] - np.float32(2.0), k0["y"], k0["x"] - np.float32(22.0)
    q["radius"] = np.float32(7.5) * sf[k0["octave"]]
    q["min_level"], q["max_level"] = k0["octave"] - 1, k0["octave"]
    q["valid"] = 1; q["blocks"] = 1; q["angle"] = k0["angle"]; q["desc"] = d0
    m = ORBmatcher(0.8, True)
    forms["proj_best"] = lambda: m.ProjBest(fv, q, inv_s2)

    groups = lambda d: {g: np.nonzero(d[:, 1] % 100 == g)[0].tolist() for g in range(100) if (d[:, 1] % 100 == g).any()}
    ga, gb = groups(d0), groups(d1)
    valid_a, valid_b = np.ones(len(d0), np.uint8), np.ones(len(d1), np.uint8)
    forms["search_by_bow"] = lambda: m.SearchByBoW(d0, k0["angle"], valid_a, ga, d1, k1["angle"], gb)
    forms["search_by_bow_kf"] = lambda: search_by_bow_kf(d0, k0["angle"], valid_a, ga, d1, k1["angle"], valid_b, gb, 0.8, True)

    R, t_ = synth.camera_pose(77)
    fr = make_frustum(R, t_, 718.856, 718.856, w / 2 + 3.2, h / 2 - 1.7, 386.1448, (0, w, 0, h), 1.2, 8)
    mp = synth.local_map(k1, d1, fr, 78, 500)
    forms["search_local_points"] = lambda: m.SearchLocalPoints(fv, fr, mp, 3.0)

    kcam = np.zeros(1, _lib.KF_CAMERA_DTYPE)
    for f in ("fx", "fy", "cx", "cy", "mbf", "min_x", "max_x", "min_y", "max_y", "log_scale_factor", "n_levels"):
        kcam[f] = fr[f]
    kcam["R"] = fr["Rcw"]; kcam["t"] = fr["tcw"]; kcam["Ow"] = fr["Ow"]; kcam["scale_factors"] = fr["scale_factors"]
    kcam["th"] = 3.0
    pts = np.zeros(len(mp), _lib.KF_POINT_DTYPE)
    for f in ("pos", "normal", "min_distance", "max_distance", "skip", "desc"):
        pts[f] = mp[f]
    forms["kf_search_fuse"] = lambda: m.KeyFrameSearch(fv, kcam, pts, _lib.KF_FUSE, inv_level_sigma2=inv_s2)
    forms["kf_search_loop"] = lambda: m.KeyFrameSearch(fv, kcam, pts, _lib.KF_LOOP, max_dist=50)

    prev = np.stack([k0["x"], k0["y"]], axis=1).astype(np.float32)
    forms["search_for_initialization"] = lambda: m.SearchForInitialization(f0, fv_mono, prev, 30)

    out = {"tag": os.environ.get("ORBFE_AB_LIB", ""), "reps": args.reps}
    for name, fn in forms.items():
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        out[name] = {"median_ms": round(ts[len(ts) // 2], 4), "p10_ms": round(ts[len(ts) // 10], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
