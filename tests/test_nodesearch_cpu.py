"""The searches over common vocabulary nodes and the initialisation search on directed input, CPU side: the C oracle against the
instrumented walks on every scene and twin of tests/np_nodesearch.py with the rotation check on and off, every placed feature at the
exit it was placed for (the builder asserts it), the census, the discriminating power of the scenes -- every one-comparison mutant of
the walks changes the result of a named scene -- and the host half of the device searches (csrc/search_plan.h), compiled as a
stand-alone program under the sanitizers (tests/cpp_nodesearch) and run on the scenes' FeatureVectors and on malformed ones.
tests/test_nodesearch_gpu.py runs the same scenes on the device."""
import operator
import os
import subprocess

import numpy as np
import pytest

from tests import np_nodesearch as nn
from tests import np_restatement as nr
from tests import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))


def oracle_result(sc, check_ori=None):
    check = sc.check_ori if check_ori is None else check_ori
    r = np.float32(sc.nnratio)
    if sc.form == "frame":
        return ol.search_by_bow(sc.descA, sc.angleA, sc.validA, sc.fvA, sc.descB, sc.angleB, sc.fvB, r, check)
    if sc.form == "kf":
        return ol.search_by_bow_kf(sc.descA, sc.angleA, sc.validA, sc.fvA, sc.descB, sc.angleB, sc.validB, sc.fvB, r, check)
    if sc.form == "tri":
        ur = (sc.urA, sc.urB) if sc.with_u_right else (None, None)
        return ol.search_for_triangulation(sc.keysA, sc.descA, ur[0], sc.hasA, sc.fvA, sc.keysB, sc.descB, ur[1], sc.hasB, sc.fvB, sc.ep,
                                           sc.only_stereo, check)
    of = ol.OracleFrame(sc.keys, sc.desc, nn.SCALE_FACTORS, 0, sc.w, 0, sc.h, None)
    return ol.search_for_initialization(sc.keys1, sc.desc1, of, sc.prev, sc.window, r, check)


def same(got, want, what):
    """got: what an implementation returns; want: the walk's tuple.  Byte for byte: counts, match arrays and (init) vbPrevMatched"""
    arrays = want[1:3] if len(want) == 5 else want[1:2]
    assert len(got) == 1 + len(arrays), what
    for g, w in zip(got[1:], arrays):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(1)) if g.shape == w.shape else None
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, None if bad is None else (bad[:8], g[bad[:8]], w[bad[:8]]))
    assert got[0] == want[0], (what, got[0], want[0])


@pytest.mark.parametrize("form", nn.FORMS)
def test_oracle_equals_walk_on_directed_scenes(form):
    for sc in nn.build_scenes(form):
        same(oracle_result(sc), sc.result, sc.name)
        same(oracle_result(sc, not sc.check_ori), sc.walk(check_ori=not sc.check_ori), sc.name + " check_ori flipped")


@pytest.mark.parametrize("form", nn.FORMS)
def test_public_readings_are_the_walk(form):
    """ref_search_by_bow / _kf / _for_triangulation / _for_initialization give what the walks give"""
    for sc in nn.build_scenes(form):
        nm, res = sc.result[:2]
        if form == "frame":
            got = nr.ref_search_by_bow(sc.descA, sc.angleA, sc.validA, sc.fvA, sc.descB, sc.angleB, sc.fvB, sc.nnratio, sc.check_ori)
        elif form == "kf":
            got = nr.ref_search_by_bow_kf(sc.descA, sc.angleA, sc.validA, sc.fvA, sc.descB, sc.angleB, sc.validB, sc.fvB, sc.nnratio, sc.check_ori)
        elif form == "tri":
            ur = (sc.urA, sc.urB) if sc.with_u_right else (None, None)
            got = nr.ref_search_for_triangulation(sc.keysA, sc.descA, ur[0], sc.hasA, sc.fvA, sc.keysB, sc.descB, ur[1], sc.hasB, sc.fvB, sc.F12,
                                                  nn.TRI_EX, nn.TRI_EY, nn.SCALE_FACTORS, nn.TRI_SIGMA2, sc.only_stereo, sc.check_ori)
        else:
            got = nr.ref_search_for_initialization(sc.keys1, sc.desc1, sc.ref_frame(), sc.prev, sc.window, sc.nnratio, sc.check_ori)
            assert np.array_equal(np.array(got[2], np.float32).reshape(-1, 2), sc.result[2]), sc.name
        assert got[0] == nm and got[1] == res.tolist(), sc.name


@pytest.mark.parametrize("form", nn.FORMS)
def test_census(form):
    """the conditions hold on the walks' own exits and facts; none of them reads a kernel's output"""
    scenes = nn.build_scenes(form)
    print(form, "directed", nn.exit_counts([sc.walk(check_ori=True)[-2:] for sc in scenes if not sc.name.endswith("+twin")], form))
    assert nn.census(scenes) == []
    if form != "init":
        assert max(len(sc.A) for sc in scenes) <= 400 and max(len(sc.fvA) + len(sc.fvB) for sc in scenes) <= 800
        assert max(len(lb) for sc in scenes for lb in sc.fvB.values()) <= 200


@pytest.mark.parametrize("form", nn.FORMS)
def test_previous_inputs_reach_less(form):
    """the gap on record: what the inputs of the undirected tests reach (the first column of the table in np_nodesearch's docstring)"""
    before = nn.exit_counts([nn.previous_inputs(form)], form)
    print(form, "before", before)
    assert before["calls with more pushes than first-side features"] == 0 and before["calls with an empty histogram"] == 0
    assert before["matched, then stolen or overwritten"] == 0 or form == "init"
    if form != "init":
        assert set(before["list or window lengths among 1, 63, 64, 65, 128, 129"]) < set(nn.LIST_LENGTHS)


def test_twins_and_sequential_scenes_are_what_they_claim():
    for form in ("frame", "kf", "tri"):
        for sc in nn.build_scenes(form):
            f = sc.result[3]
            seq = f["dup_a"] if form == "tri" else f["dup_b"] or (form == "kf" and f["dup_a"])
            if form == "frame" and sc.name.startswith("dup_a"):
                assert f["dup_a"] and not seq, sc.name      # a repeated keyframe feature couples nothing in the KF-Frame form
            elif form == "tri" and sc.name == "dup_b":
                assert not seq, sc.name                     # nothing is ever taken in SearchForTriangulation
            else:
                assert bool(seq) == (sc.name.endswith("+twin") or sc.sequential_only), (form, sc.name)
        by_name = {s.name: s for s in nn.build_scenes(form)}
        f = by_name["dup_a"].result[3]
        a1 = by_name["dup_a"].tags["dup_a"][0]
        assert f["pushes"][a1] == 3 and [v["exit"] for v in f["visits"] if v["a"] == a1][1] == nn.NX_ROTATION
        assert int(by_name["dup_a_only"].result[3]["pushes"].sum()) == 5 > len(by_name["dup_a_only"].A)
        if form != "frame":     # the slot is cleared through the middle visit's entry although the last visit's bin was kept
            assert by_name["dup_a"].result[1][a1] == -1 and by_name["dup_a"].walk(check_ori=False)[1][a1] >= 0


# One comparison of a walk swapped at a time: (what is swapped, the rule, the form and scene that must notice).  No kernel mutant is
# built or run; this shows that the scenes would tell such a kernel from the reference.
le, lt, ge, gt = operator.le, operator.lt, operator.ge, operator.gt
MUTANTS = [
    ("KF-Frame accepts only < TH_LOW", dict(accept_frame=lt), "frame", "thresholds"),
    ("KF-KF accepts <= TH_LOW", dict(accept_kf=le), "kf", "thresholds"),
    ("initialisation accepts only < TH_LOW", dict(accept_init=lt), "init", "init_basic"),
    ("ratio <= (KF-Frame)", dict(ratio_lt=le), "frame", "ratio_0.75"),
    ("ratio <= (KF-KF)", dict(ratio_lt=le), "kf", "ratio_0.9"),
    ("ratio <= (initialisation)", dict(ratio_lt=le), "init", "init_basic"),
    ("ratio as a double product", dict(ratio_float=False), "frame", "ratio_0.6"),
    ("triangulation rejects dist >= TH_LOW", dict(tri_far=ge), "tri", "tri_lists"),
    ("triangulation: the first of equal candidates wins", dict(tri_worse=ge), "tri", "tri_lists"),
    ("u_right > 0", dict(has_right=lambda ur: ur > 0), "tri", "tri_disc"),
    ("epipole disc <=", dict(disc_lt=le), "tri", "tri_disc"),
    ("epipole disc in double", dict(disc_float=False), "tri", "tri_disc"),
    ("epipolar gate <=", dict(epi_lt=le), "tri", "tri_epipolar"),
    ("epipolar gate in float", dict(epi_double=False), "tri", "tri_epipolar"),
    ("an equal distance steals", dict(kept_le=lt), "init", "init_steal"),
    ("a stolen match leaves the histogram", dict(stolen_stay_in_hist=False), "init", "init_hist_stolen"),
    ("round half to even", dict(round=lambda x: int(np.rint(np.float32(x)))), "frame", "rot_bounds"),
] + [(f"{what} ({form})", rule, form, scene) for form in nn.FORMS for what, rule, scene in (
    ("three_maxima: s >= max1", dict(max_gt1=ge), "rot_tie4"),
    ("three_maxima: s >= max2", dict(max_gt2=ge), "rot_tie_second"),
    ("three_maxima: s >= max3", dict(max_gt3=ge), "rot_tie_third"),
    ("three_maxima: max2 <= 0.1f * max1", dict(max_lt2=le), "rot_10_1"),
    ("three_maxima: max3 <= 0.1f * max1", dict(max_lt3=le), "rot_third_kept"))]

# Comparisons whose swap cannot change a result, so that no scene can notice it:
#   best_lt / second_lt in SearchByBoW and SearchForInitialization: with `<=` a later candidate of equal distance becomes the best and the
#     earlier one the second-best -- the two distances are the same pair as before, and since best == second the ratio test (ratio < 1)
#     rejects either way; a tie for the second-best leaves the second-best DISTANCE alone.  (SearchForTriangulation has no ratio test, and
#     there the tie rule is the mutant "the first of equal candidates wins".)
#   den_zero: without the test dsqr is +inf or nan, and `dsqr < 3.84 * sigma2` is false for both.
EQUIVALENT = [("best <=", dict(best_lt=le)), ("second-best <=", dict(second_lt=le)), ("no den == 0 test", dict(den_zero=lambda den: False))]


@pytest.mark.parametrize("what,rule,form,scene", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_mutant_of_the_walks_is_noticed(what, rule, form, scene):
    assert set(rule) <= set(nr.NODE_RULES)
    sc = {s.name: s for s in nn.build_scenes(form)}[scene]
    want = sc.result
    got = sc.walk(rules=dict(nr.NODE_RULES, **rule))
    assert (got[0], got[1].tobytes()) != (want[0], want[1].tobytes()), (what, scene)


def test_no_rule_is_left_without_a_mutant():
    covered = set().union(*[set(m[1]) for m in MUTANTS]) | set().union(*[set(e[1]) for e in EQUIVALENT])
    assert covered == set(nr.NODE_RULES)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("what,rule", EQUIVALENT, ids=[e[0] for e in EQUIVALENT])
def test_equivalent_mutants_change_nothing(what, rule):
    for form in nn.FORMS:
        if form == "tri" and "den_zero" not in rule or form != "tri" and "den_zero" in rule:
            continue
        for sc in nn.build_scenes(form):
            got = sc.walk(rules=dict(nr.NODE_RULES, **rule))
            assert (got[0], got[1].tobytes()) == (sc.result[0], sc.result[1].tobytes()), (what, form, sc.name)


# ---- the host half of the device searches ---------------------------------------------------------------------------------------------
MODES = {"frame": 0, "kf": 1, "tri": 2}


def _case_text(name, mode, nA, nB, nodesA, idxA, nodesB, idxB):
    flat = lambda nodes: " ".join(f"{a} {b} {c}" for a, b, c in nodes)
    return (f"{name} {mode} {nA} {nB} {len(nodesA)} {len(nodesB)} {len(idxA)} {len(idxB)}\n{flat(nodesA)}\n{' '.join(map(str, idxA))}\n"
            f"{flat(nodesB)}\n{' '.join(map(str, idxB))}\n")


def _flatten(fv):
    nodes, idx = [], []
    for nid in sorted(fv):
        nodes.append((nid, len(idx), len(fv[nid])))
        idx.extend(fv[nid])
    return nodes, idx


def _run_plan(tmp_path, text):
    exe = os.path.join(HERE, "cpp_nodesearch", "_build", "plan_check")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp_nodesearch")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    path = tmp_path / "cases.txt"
    path.write_text(text)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]     # a sanitizer report ends the program with an error
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("cases="):
            out["cases"] = int(line[6:])
            continue
        head, pairs = line.split(" :")
        f = head.split()
        out[f[0]] = dict({k: int(v) for k, v in (kv.split("=") for kv in f[1:])},
                         pair_list=[tuple(map(int, p.split(","))) for p in pairs.replace(";", " ").split()])
    return out


def test_plan_program_on_the_scenes(tmp_path):
    """pair list, sequential flag and scratch capacity of csrc/search_plan.h against what the walks need: the pairs of the reference's
    lock-step walk, the replay wherever a recurring feature couples two visits, and room for every push of the histogram"""
    cases, text = {}, []
    for form, mode in MODES.items():
        for sc in nn.build_scenes(form):
            name = f"{form}:{sc.name}".replace(" ", "_")
            nodesA, idxA = _flatten(sc.fvA)
            nodesB, idxB = _flatten(sc.fvB)
            cases[name] = (sc, nodesA, nodesB)
            text.append(_case_text(name, mode, len(sc.A), len(sc.B), nodesA, idxA, nodesB, idxB))
    out = _run_plan(tmp_path, "".join(text))
    assert out["cases"] == len(cases)
    for name, (sc, nodesA, nodesB) in cases.items():
        got, f = out[name], sc.walk(check_ori=True)[3]
        startA, startB = {n[0]: n[1] for n in nodesA}, {n[0]: n[1] for n in nodesB}
        want_pairs = [(startA[nid], len(la), startB[nid], len(lb)) for nid, la, lb in nr._featvec_pairs(sc.fvA, sc.fvB)]
        assert got["rc"] == 0 and got["pair_list"] == want_pairs and got["pairs"] == f["n_pairs"], name
        assert got["maxB"] == max([p[3] for p in want_pairs] + [0]) and got["totA"] == sum(n[2] for n in nodesA), name
        coupled = f["dup_a"] if sc.form == "tri" else f["dup_b"] or (sc.form == "kf" and f["dup_a"])
        assert got["sequential"] == int(bool(coupled)), (name, "a feature recurs among the pairs and the replay is off" if coupled else "")
        assert got["push_cap"] >= int(f["pushes"].sum()), (name, "the histogram takes more entries than the scratch holds",
                                                            got["push_cap"], int(f["pushes"].sum()))
        assert got["push_cap"] >= len(sc.A) and got["push_cap"] >= len(f["visits"]), name


def test_plan_program_refuses_malformed_feature_vectors(tmp_path):
    ok = ([(5, 0, 2), (9, 2, 1)], [0, 1, 2], [(5, 0, 2), (9, 2, 2)], [0, 1, 2, 3])
    bad = {
        "index_a_negative": (ok[0], [0, -1, 2], ok[2], ok[3]),
        "index_a_too_large": (ok[0], [0, 1, 3], ok[2], ok[3]),
        "index_b_negative": (ok[0], ok[1], ok[2], [0, 1, -5, 3]),
        "index_b_too_large": (ok[0], ok[1], ok[2], [0, 1, 2, 4]),
        "start_a_negative": ([(5, -1, 2), (9, 2, 1)], ok[1], ok[2], ok[3]),
        "count_a_negative": ([(5, 0, -2), (9, 2, 1)], ok[1], ok[2], ok[3]),
        "start_b_negative": (ok[0], ok[1], [(5, -3, 2), (9, 2, 2)], ok[3]),
        "count_b_negative": (ok[0], ok[1], [(5, 0, 2), (9, 2, -1)], ok[3]),
        "node_of_60001": (ok[0], ok[1], [(5, 0, 60001), (9, 2, 2)], ok[3]),
    }
    text = [_case_text("ok", 0, 3, 4, *ok), _case_text("bad_only_in_an_unshared_node", 1, 3, 4, [(4, 0, 1), (5, 1, 2)], [7, 1, 2], ok[2], ok[3])]
    for name, c in bad.items():
        for mode in (0, 1, 2):
            text.append(_case_text(f"{name}:{mode}", mode, 3, 4, *c))
    # legal but odd: two nodes name the SAME range of the index array, so two first-side features are visited four times -- more
    # visits than the array has entries.  Each visit can push, so the scratch must hold four; the feature recurs among the pairs.
    overlap = ([(5, 0, 2), (9, 0, 2)], [0, 1], [(5, 0, 2), (9, 2, 2)], [0, 1, 2, 3])
    for mode in (0, 1, 2):
        text.append(_case_text(f"overlap:{mode}", mode, 2, 4, *overlap))
    out = _run_plan(tmp_path, "".join(text))
    assert out["ok"]["rc"] == 0 and out["ok"]["pairs"] == 2 and out["ok"]["sequential"] == 0
    for mode in (0, 1, 2):
        o = out[f"overlap:{mode}"]
        assert o["rc"] == 0 and o["totA"] == 2 and o["push_cap"] >= 4 and o["sequential"] == int(mode != 0), (mode, o)
    assert out["bad_only_in_an_unshared_node"]["rc"] == 0      # node 4 has no partner: its list is never read
    for name in bad:
        for mode in (0, 1, 2):
            assert out[f"{name}:{mode}"]["rc"] == -1, (name, mode)
