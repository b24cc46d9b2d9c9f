"""The ordered projection searches on directed input, CPU side: the C oracle against the instrumented walk on every scene of
tests/np_projection.py, every hand-placed query at the exit it was placed for (the builder asserts it), the census -- the proof that
the directed input reaches what extracted frames with jitter do not (dependency chains of depth 200, claims given up, ties decided by
cell order, every threshold at equality, the list lengths at which the resolver changes its path, a full staging area) -- and the
discriminating power of the scenes: every one-comparison mutant of the walk changes the result of a named scene.
tests/test_projection_gpu.py runs the same scenes on the device."""
import operator

import numpy as np
import pytest

from tests import np_projection as npj
from tests import np_restatement as nr
from tests import oracle_lib as ol

CASES = [(form, geom) for form in npj.FORMS for geom in npj.GEOMETRIES]


def oracle_frame(sc):
    return ol.OracleFrame(sc.keys, sc.desc, npj.SCALE_FACTORS, 0, sc.w, 0, sc.h, sc.u_right if sc.has_u_right else None)


def oracle_result(sc, queries=None, check_ori=None):
    q = sc.queries if queries is None else queries
    check = sc.check_ori if check_ori is None else check_ori
    of = oracle_frame(sc)
    if sc.form == "points":
        return of.search_by_projection_points(q, np.float32(sc.nnratio), sc.blocked0)
    if sc.form == "frame":
        return of.search_by_projection_frame(q, check, sc.blocked0)
    return of.search_by_projection_keyframe(q, check, npj.ORB_DIST, sc.blocked0)


@pytest.mark.parametrize("form,geom", CASES)
def test_oracle_equals_walk_on_directed_scenes(form, geom):
    for sc in npj.build_scenes(form, *geom):
        nm, assigned, blocked = sc.result[:3]
        onm, oassigned, oblocked = oracle_result(sc)
        assert onm == nm and oassigned.tobytes() == assigned.tobytes() and oblocked.tobytes() == blocked.tobytes(), sc.name
        if sc.form != "points":      # and with the rotation check the other way round
            nm, assigned, blocked = sc.walk(check_ori=not sc.check_ori)[:3]
            onm, oassigned, oblocked = oracle_result(sc, check_ori=not sc.check_ori)
            assert onm == nm and oassigned.tobytes() == assigned.tobytes() and oblocked.tobytes() == blocked.tobytes(), sc.name


@pytest.mark.parametrize("form,geom", CASES)
def test_public_readings_are_the_walk(form, geom):
    """ref_search_by_projection_points / _frame / _keyframe on the scenes they can express give what proj_walk gives"""
    for sc in npj.build_scenes(form, *geom):
        q = sc.queries
        F = sc.ref_frame()
        if form == "points":
            if not np.all(q["min_level"][q["valid"] != 0] == q["max_level"][q["valid"] != 0] - 1):
                continue     # the reading takes one level per point and searches level - 1 .. level
            pts = [dict(skip=not e["valid"], proj_x=e["u"], proj_y=e["v"], proj_xr=e["u_r"], level=int(e["max_level"]), radius=e["radius"],
                        observed=bool(e["blocks"]), desc=e["desc"]) for e in q]
            got = nr.ref_search_by_projection_points(F, pts, sc.nnratio, sc.blocked0)
        else:
            last = [dict(skip=not e["valid"], u=e["u"], v=e["v"], ur=e["u_r"], radius=e["radius"], min_level=int(e["min_level"]),
                         max_level=int(e["max_level"]), observed=bool(e["blocks"]), angle=e["angle"], desc=e["desc"]) for e in q]
            if form == "frame":
                got = nr.ref_search_by_projection_frame(F, last, sc.check_ori, sc.blocked0)
            else:
                F.u_right = None
                got = nr.ref_search_by_projection_keyframe(F, last, npj.ORB_DIST, sc.check_ori, sc.blocked0)
        nm, assigned, blocked = sc.result[:3]
        assert got[0] == nm and got[1] == assigned.tolist() and [int(b) for b in got[2]] == blocked.tolist(), sc.name


@pytest.mark.parametrize("form,geom", CASES)
def test_census(form, geom):
    """the conditions hold on the walk's own exits and facts; none of them reads the kernel's output"""
    scenes = npj.build_scenes(form, *geom)
    print(form, geom, npj.exit_counts([sc.result[3:] for sc in scenes]))
    assert npj.census(scenes) == []
    assert max(len(sc.keys) for sc in scenes) <= 2600 and max(len(sc.queries) for sc in scenes) <= 2300
    by_name = {sc.name: sc for sc in scenes}
    f = by_name["windows"].result[4]
    t = by_name["windows"].tags
    assert f["ncol"][t["cols17"][0]] == 17 and f["ncol"][t["cols64"][0]] == 64
    assert all(f["ncol"][i] < 6 for i in t["clipped"]) and all(f["ncol"][i] == 0 for i in t["outside"])
    f = by_name["listlen"].result[4]
    t = by_name["listlen"].tags
    assert [f["n_window"][i] for i in t["kept5"] + t["kept4"] + t["raw6"] + t["full64"]] == [5, 4, 6, 6, 64]
    assert [f["matters_kept"][i] for i in t["kept5"] + t["kept4"] + t["raw6"]] == [5, 4, 4, 4]
    assert all(f["n_window"][i] == 65 for i in t["trunc"] + t["trunc_after_chunk"] + t["second_same_batch"] + t["second_later_batch"])
    assert f["n_blocked_by_call"][t["trunc_after_chunk"][0]] == 2
    assert (f["second_pos"][t["second_same_batch"][0]], f["second_pos"][t["second_later_batch"][0]]) == (5, 64)
    C = npj.kernel_constants()
    cut = npj.chunks(by_name["staging"].result[4]["n_window"], C)
    per = C["ORBFE_MAX_CAND"] - C["RC_REG"]       # 300 queries of 64 candidates each: the first chunk takes what fits the staging area
    assert cut == [(0, C["RC_LIST_CAP"] // per, C["RC_LIST_CAP"] // per * per), (C["RC_LIST_CAP"] // per, 300 - C["RC_LIST_CAP"] // per,
                                                                                  (300 - C["RC_LIST_CAP"] // per) * per)], cut
    assert by_name["chain"].result[4]["depth"].max() == 204


def test_kernel_constants_are_found():
    assert npj.kernel_constants() == dict(RC_THREADS=1024, RC_REG=4, RC_LIST_CAP=16384, ORBFE_CAND_LANES=16, ORBFE_MAX_CAND=64)


@pytest.mark.parametrize("geom", npj.GEOMETRIES)
def test_features_in_area_on_the_windows_scene(geom):
    """oo_features_in_area equals the second reading of Frame::GetFeaturesInArea, order included, for every query of the windows scene"""
    for form in ("frame", "points"):
        sc = {s.name: s for s in npj.build_scenes(form, *geom)}["windows"]
        of, F = oracle_frame(sc), sc.ref_frame()
        hit = 0
        for q in sc.queries:
            a = of.features_in_area(float(q["u"]), float(q["v"]), float(q["radius"]), int(q["min_level"]), int(q["max_level"]))
            b = F.GetFeaturesInArea(q["u"], q["v"], q["radius"], int(q["min_level"]), int(q["max_level"]))
            assert list(a) == b, (form, q)
            hit += len(b) > 0
        assert hit >= 20


def test_reversed_queries_change_the_result():
    """the order of the queries decides: the chain scene walked backwards matches other keypoints (and the oracle follows)"""
    for form in npj.FORMS:
        sc = npj.build_scenes(form)[0]
        assert sc.name == "chain"
        rq = sc.queries[::-1].copy()
        nm, assigned, blocked = sc.walk(rq)[:3]
        onm, oassigned, oblocked = oracle_result(sc, rq)
        assert onm == nm and oassigned.tobytes() == assigned.tobytes() and oblocked.tobytes() == blocked.tobytes()
        back = np.where(assigned >= 0, len(rq) - 1 - assigned, -1)
        assert not np.array_equal(back, sc.result[1])


# One comparison of the walk swapped at a time: (what is swapped, the rule, the form and scene that must notice).  No kernel mutant is
# built or run; this shows that the scenes would tell such a kernel from the reference.
MUTANTS = [
    ("best tie <=", dict(best_lt=operator.le), "frame", "ties"),
    ("dist < th_high", dict(accept=operator.lt), "frame", "thresholds"),
    ("dist < ORBdist", dict(accept=operator.lt), "keyframe", "thresholds"),
    ("ratio >=", dict(ratio_reject=operator.ge), "points", "ratio05"),
    ("ratio ignoring the level", dict(same_level=lambda a, b: True), "points", "ratio05"),
    ("second-best level of the later tied candidate", dict(second_lt=operator.le), "points", "ties"),
    ("first taker wins", dict(last_taker_wins=False), "frame", "chain"),
    ("a non-blocking match blocks", dict(blocks=lambda b: True), "points", "staging"),
    ("rotation removal leaves blocked set", dict(rot_unblocks=False), "frame", "rot_11_1"),
    ("rotation removal clears only the last taker's entry", dict(rot_clears_all=False), "frame", "rot_11_1"),
    ("box <=", dict(in_box=operator.le), "frame", "windows"),
    ("stereo gate >=", dict(gate_fail=operator.ge), "frame", "windows"),
    ("gate on u_right >= 0", dict(has_right=lambda ur: ur >= 0), "points", "windows"),
    ("0.1 rule <=", dict(maxima_lt=operator.le), "frame", "rot_10_1"),
    ("0.1 rule <= for the third maximum", dict(maxima_lt=operator.le), "keyframe", "rot_third_kept"),
    ("round half to even", dict(round=lambda x: int(np.rint(np.float32(x)))), "frame", "rot_11_1"),
]


@pytest.mark.parametrize("what,rule,form,scene", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_mutant_of_the_walk_is_noticed(what, rule, form, scene):
    assert set(rule) <= set(nr.PROJ_RULES)
    for geom in npj.GEOMETRIES:
        sc = {s.name: s for s in npj.build_scenes(form, *geom)}[scene]
        nm, assigned, blocked = sc.result[:3]
        mnm, massigned, mblocked = sc.walk(rules=dict(nr.PROJ_RULES, **rule))[:3]
        assert (mnm, massigned.tobytes(), mblocked.tobytes()) != (nm, assigned.tobytes(), blocked.tobytes()), (what, scene, geom)
