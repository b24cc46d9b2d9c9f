"""CPU suite of the essential-graph optimisation (Optimizer::OptimizeEssentialGraph) and the map correction behind it: the numpy
reading (tests/np_egraph.py) against itself -- two solves, a permuted summation order, 4 ulp of noise on every summand --, which
fixes the parity bound of tests/test_egraph_gpu.py; the arithmetic of csrc/egraph_internal.h compiled for the host against the
reading; the limits, the record sizes and the envelope count of the C ABI, all of which answer before a device is looked for."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer, sim3
from tests import np_egraph as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNING = [n for n in G.CASES if n not in ("edges_0", "no_free", "n_kf_1")]


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def host():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_egraph")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return C.CDLL(os.path.join(ROOT, "tests", "cpp_egraph", "_build", "libegraph_host.so"))


_runs = {}


def four_runs(name):
    """envelope solve, dense solve, permuted summation order, 4 ulp of relative noise on every summand: computed once per case"""
    if name not in _runs:
        s = G.case_scene(name)
        _runs[name] = (s, [G.run_case(s), G.run_case(s, solve="dense"), G.run_case(s, order_seed=11),
                           G.run_case(s, order_seed=12, noise=4 * G.ULP)])
    return _runs[name]


def spread_units(runs):
    worst = 0.0
    for r in runs[1:]:
        worst = max(worst, G.sim3_units(r["sim3"], runs[0]["sim3"]), G.pose_units(r["poses"], runs[0]["poses"]))
    return worst


@pytest.mark.parametrize("name", RUNNING)
def test_stability_and_bound(name):
    """The four runs decide every accept / reject alike, and their outputs spread by at most a quarter of the bound of their path
    (np_egraph.BOUND_UNITS, in units of the library's criterion).  Prints the smallest |rho| and the spread."""
    s, runs = four_runs(name)
    spread = spread_units(runs)
    print(f"{name}: iterations {runs[0]['iterations']} trials {runs[0]['trials']} min |rho| {min(r['min_rho'] for r in runs):.3g} "
          f"spread {spread:.3g} units")
    for r in runs[1:]:
        assert r["decisions"] == runs[0]["decisions"], (name, r["rhos"], runs[0]["rhos"])
        assert r["iterations"] == runs[0]["iterations"] and r["status"] == runs[0]["status"] == 0
    assert runs[0]["iterations"] >= 1 and any(runs[0]["decisions"])
    assert runs[0]["chi2_last"] < runs[0]["chi2_first"]
    assert spread <= G.BOUND_UNITS[s["fix_scale"]] / 4


def test_bound_constants_follow_the_measurement():
    """BOUND_UNITS is 1 where the recorded spread is at most a quarter, else four times it; the recorded spread is not below what the
    cases measure now"""
    for fs in (False, True):
        m = G.MEASURED_SPREAD_UNITS[fs]
        assert G.BOUND_UNITS[fs] == (1.0 if m <= 0.25 else 4 * m)
        worst = max(spread_units(four_runs(n)[1]) for n in RUNNING if G.case_scene(n)["fix_scale"] == fs)
        assert worst <= m, (fs, worst)


def test_cases_are_what_their_names_promise():
    s = G.case_scene("chain6")
    assert len(s["vertices"]) == 6 and len(s["edges"]) == 6 and s["vertices"]["fixed"].tolist() == [1, 0, 0, 0, 0, 0]
    assert (s["edges"]["kind"] == G.LOOP_CONNECTION).sum() == 1 and tuple(s["edges"][0]) == (5, 0, 1)
    assert abs(s["vertices"]["Scw"]["s"][5] - 1.1) < 1e-12 and not s["fix_scale"]
    s = G.case_scene("band")
    d = np.abs(s["edges"]["i"] - s["edges"]["j"])
    assert len(s["vertices"]) == 40 and sorted(set(d[s["edges"]["kind"] == 0].tolist())) == [1, 2, 3, 17, 19]
    s, runs = four_runs("fixed_mid")
    fixed = np.flatnonzero(s["vertices"]["fixed"])
    assert fixed.tolist() == [5] and runs[0]["n_free"] == 11
    assert runs[0]["sim3"][5].tobytes() == s["vertices"]["Scw"][5].tobytes()
    s, runs = four_runs("two_fixed")
    assert np.flatnonzero(s["vertices"]["fixed"]).tolist() == [0, 4] and runs[0]["n_free"] == 8
    s, runs = four_runs("isolated")
    assert 4 not in s["edges"]["i"] and 4 not in s["edges"]["j"] and not s["vertices"]["fixed"][4]
    assert runs[0]["sim3"][4].tobytes() == s["vertices"]["Scw"][4].tobytes() and runs[0]["n_free"] == 7
    # a start far from the optimum (the Sim3 form's chi2 drops by two orders of magnitude) and rejected trials; with lambda starting at
    # 1e-16 a rejection is a repeated Gauss-Newton step, so only the SE3 case, whose tenth trial is damped enough, accepts one after it
    for name, drop in (("rejected_step", 100.0), ("rejected_step_se3", 1.0)):
        r = four_runs(name)[1][0]
        assert False in r["decisions"] and r["chi2_first"] > drop * r["chi2_last"], r["decisions"]
    dec = four_runs("rejected_step_se3")[1][0]["decisions"]
    assert True in dec[dec.index(False):], dec
    for name in ("edges_0", "no_free", "n_kf_1"):
        s = G.case_scene(name)
        r = G.run_case(s)
        assert r["iterations"] == 0 and r["trials"] == 0 and r["sim3"].tobytes() == s["vertices"]["Scw"].tobytes()
    s = G.case_scene("wide")
    assert len(s["vertices"]) == 300 and four_runs("wide")[1][0]["envelope_blocks"] > 299 * 9


@pytest.mark.parametrize("name", ["chain6", "band", "rejected_step", "chain6_se3", "band_se3", "fixed_mid_se3", "wide"])
def test_host_arithmetic_against_the_reading(host, name):
    """csrc/egraph_internal.h compiled for the host: measurements and errors to the last bits, the analytic Jacobian to rounding, the
    numeric one to the noise of its difference quotient (an ulp of the error over the step 1e-9), oplus and the pose rows"""
    s = G.case_scene(name)
    V, E, se3 = s["vertices"], s["edges"], s["fix_scale"]
    n = len(E)
    meas, err, Ji, Jj = np.zeros((n, 8)), np.zeros((n, 7)), np.zeros((n, 49)), np.zeros((n, 49))
    host.egraph_host_linearize(_lib.ptr(V), _lib.ptr(E), n, int(se3), _lib.ptr(meas), _lib.ptr(err), _lib.ptr(Ji), _lib.ptr(Jj))
    g = G._Graph(V, E, se3)
    D = g.D
    ref_meas = np.stack(list(g.C[0]) + list(g.C[1]) + [g.C[2]], 1)
    e_ref = g.errors(g.est)
    A, B = g.jacobians(g.est)
    assert np.abs(meas - ref_meas).max() <= 4 * G.ULP * max(1.0, np.abs(ref_meas).max())
    assert np.abs(err[:, :D] - e_ref).max() <= 16 * G.ULP * max(1.0, np.abs(e_ref).max())
    ji = Ji[:, :D * D].reshape(n, D, D).transpose(0, 2, 1)
    jj = Jj[:, :D * D].reshape(n, D, D).transpose(0, 2, 1)
    tol = 64 * G.ULP * max(1.0, np.abs(A).max()) if se3 else 16 * G.ULP * max(1.0, np.abs(e_ref).max()) / (2 * 1e-9) * 4
    assert np.abs(ji - A).max() <= tol and np.abs(jj - B).max() <= tol
    rng = np.random.default_rng(3)
    for k in range(min(4, len(V))):
        x = rng.normal(size=D) * 0.1
        out = np.zeros(1, _lib.EG_SIM3_DTYPE)
        host.egraph_host_oplus(_lib.ptr(V["Scw"][k:k + 1].copy()), _lib.ptr(x), int(se3), _lib.ptr(out))
        est = [a.copy() for a in g.est]
        g.oplus(est, k, x)
        ref = np.concatenate([est[0][k], est[1][k], [est[2][k]]])
        got = np.concatenate([out["q"][0], out["t"][0], out["s"]])
        assert np.abs(got - ref).max() <= 16 * G.ULP * max(1.0, np.abs(ref).max())
    poses = np.zeros((len(V), 12), np.float32)
    host.egraph_host_poses(_lib.ptr(np.ascontiguousarray(V["Scw"])), len(V), int(se3), _lib.ptr(poses))
    assert np.array_equal(poses, G.poses_of(V["Scw"], se3))


def test_host_correct_points_against_the_reading(host):
    pts, ref, a, b = correct_points_scene()
    out = np.zeros_like(pts)
    host.egraph_host_correct_points(_lib.ptr(pts), len(pts), _lib.ptr(ref), _lib.ptr(a), _lib.ptr(b), _lib.ptr(out))
    want = G.correct_points(pts, ref, a, b)
    assert np.array_equal(out[ref < 0], pts[ref < 0])
    assert G.point_units(out, want) <= 1.0 and (out != want).mean() < 0.01     # one rounding to float: the doubles differ by ulps


def correct_points_scene():
    """1 000 points over the 8 tables of the chain of a graph: vScw and a corrected Siw per keyframe, ref including the fixed
    keyframe 0 and -1"""
    s = G.make_scene(21, n_kf=8, band=2, n_corrected=2)
    r = G.run_case(s)
    rng = np.random.default_rng(5)
    pts = (rng.normal(size=(1000, 3)) * 8).astype(np.float32)
    ref = rng.integers(-1, 8, 1000).astype(np.int32)
    ref[:4] = [0, -1, 7, 0]
    return pts, ref, np.ascontiguousarray(s["vertices"]["Scw"]), np.ascontiguousarray(r["sim3"])


def test_record_sizes_and_constants():
    assert _lib.EG_SIM3_DTYPE.itemsize == 64 and _lib.EG_VERTEX_DTYPE.itemsize == 136 and _lib.EG_EDGE_DTYPE.itemsize == 12
    assert _lib.EG_PROBLEM_DTYPE.itemsize == 16 and _lib.EG_RESULT_DTYPE.itemsize == 48
    assert G.SIM3_DTYPE == _lib.EG_SIM3_DTYPE and G.VERTEX_DTYPE == _lib.EG_VERTEX_DTYPE and G.EDGE_DTYPE == _lib.EG_EDGE_DTYPE
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for name, val in (("MAX_KEYFRAMES", _lib.EG_MAX_KEYFRAMES), ("MAX_EDGES", _lib.EG_MAX_EDGES),
                      ("MAX_ENVELOPE_BLOCKS", _lib.EG_MAX_ENVELOPE_BLOCKS), ("MAX_PROBLEMS", _lib.EG_MAX_PROBLEMS),
                      ("FIX_SCALE", _lib.EG_FIX_SCALE), ("LOOP_CONNECTION", _lib.EG_LOOP_CONNECTION), ("NORMAL", _lib.EG_NORMAL),
                      ("FACTOR_FAILED", _lib.EG_FACTOR_FAILED)):
        assert f"#define ORBFE_EG_{name} {val}" in hdr, name
    assert "#define ORBFE_EG_REFUSED (-1)" in hdr and _lib.EG_REFUSED == -1


@pytest.mark.parametrize("name", list(G.CASES))
def test_envelope_blocks_against_brute_force(L, name):
    s = G.case_scene(name)
    fixed = (s["vertices"]["fixed"] != 0).astype(np.uint8)
    got = optimizer.essential_graph_envelope_blocks(len(fixed), fixed, s["edges"])
    assert got == G.envelope_blocks_brute(len(fixed), fixed, s["edges"]) == G.envelope(len(fixed), fixed, s["edges"])[2]
    assert optimizer.essential_graph_envelope_blocks(len(fixed), None, s["edges"]) == \
        G.envelope_blocks_brute(len(fixed), None, s["edges"])


def test_envelope_blocks_random_graphs(L):
    rng = np.random.default_rng(7)
    for _ in range(40):
        n = int(rng.integers(2, 30))
        m = int(rng.integers(0, 60))
        e = np.zeros(m, _lib.EG_EDGE_DTYPE)
        e["i"] = rng.integers(0, n, m)
        e["j"] = (e["i"] + rng.integers(1, n, m)) % n
        fixed = (rng.uniform(size=n) < 0.2).astype(np.uint8)
        assert optimizer.essential_graph_envelope_blocks(n, fixed, e) == G.envelope_blocks_brute(n, fixed, e)


def _rc(fn, *a):
    with pytest.raises(_lib.OrbfeError) as ei:
        fn(*a)
    return ei.value.code


def test_limits_and_argument_errors(L):
    """Every limit answers ORBFE_ERR_INVALID before a device is looked for"""
    s = G.case_scene("chain6")
    V, E = s["vertices"], s["edges"]
    inv = _lib.ERR_INVALID

    def bad_vertex(field, sub, idx, value):
        W = V.copy()
        if sub is None:
            W[field]["s"][2] = value
        else:
            W[field][sub][2, idx] = value
        return W

    for W in (bad_vertex("Scw", None, 0, 0.0), bad_vertex("Snc", None, 0, -1.0), bad_vertex("Scw", None, 0, math.nan),
              bad_vertex("Scw", "t", 1, math.inf), bad_vertex("Snc", "q", 3, math.nan)):
        assert _rc(optimizer.essential_graph, W, E) == inv
    W = V.copy()
    W["Scw"]["q"][3] = 0.0
    assert _rc(optimizer.essential_graph, W, E) == inv                      # a quaternion of norm 0
    for i, j, kind in ((6, 0, 0), (-1, 0, 0), (0, 6, 0), (2, 2, 0), (1, 0, 2)):
        F = E.copy()
        F[1] = (i, j, kind)
        assert _rc(optimizer.essential_graph, V, F) == inv
        if kind == 0:
            assert _rc(optimizer.essential_graph_envelope_blocks, 6, None, F) == inv
    lib = _lib.lib()
    res = np.zeros(1, _lib.EG_RESULT_DTYPE)
    so, po = np.zeros(6, _lib.EG_SIM3_DTYPE), np.zeros((6, 12), np.float32)
    p = _lib.ptr
    assert lib.orbfe_essential_graph(p(V), 6, p(E), 6, 2, p(so), p(po), p(res)) == inv             # unknown flag
    assert lib.orbfe_essential_graph(p(V), -1, p(E), 6, 0, p(so), p(po), p(res)) == inv
    assert lib.orbfe_essential_graph(p(V), 6, p(E), -1, 0, p(so), p(po), p(res)) == inv
    assert lib.orbfe_essential_graph(p(V), _lib.EG_MAX_KEYFRAMES + 1, p(E), 6, 0, p(so), p(po), p(res)) == inv
    assert lib.orbfe_essential_graph(p(V), 6, p(E), _lib.EG_MAX_EDGES + 1, 0, p(so), p(po), p(res)) == inv
    assert lib.orbfe_essential_graph(None, 6, p(E), 6, 0, p(so), p(po), p(res)) == inv
    assert lib.orbfe_essential_graph(p(V), 6, None, 6, 0, p(so), p(po), p(res)) == inv
    assert lib.orbfe_essential_graph(p(V), 6, p(E), 6, 0, None, p(po), p(res)) == inv
    assert lib.orbfe_essential_graph(p(V), 6, p(E), 6, 0, p(so), p(po), None) == inv
    # the SE3 path: a record and a derived measurement beyond |s - 1| <= 1e-3
    s3 = G.case_scene("chain6_se3")
    W = s3["vertices"].copy()
    W["Scw"]["s"][3] = 1 + 2e-3
    assert _rc(optimizer.essential_graph, W, s3["edges"], True) == inv and not G.valid(W, s3["edges"], True)
    W = s3["vertices"].copy()
    W["Snc"]["s"][2], W["Snc"]["s"][3] = 1 + 8e-4, 1 - 8e-4                 # each within the tolerance, their quotient not
    assert _rc(optimizer.essential_graph, W, s3["edges"], True) == inv and not G.valid(W, s3["edges"], True)
    # workspace and batch arguments
    n = C.c_size_t(0)
    assert optimizer.essential_graph_workspace_bytes(0, 6, 6, 9) == 0
    assert optimizer.essential_graph_workspace_bytes(2, 6, 6, 9) == 2 * optimizer.essential_graph_workspace_bytes(1, 6, 6, 9)
    for args in ((-1, 6, 6, 9), (_lib.EG_MAX_PROBLEMS + 1, 6, 6, 9), (1, _lib.EG_MAX_KEYFRAMES + 1, 6, 9), (1, 6, _lib.EG_MAX_EDGES + 1, 9),
                 (1, 6, 6, _lib.EG_MAX_ENVELOPE_BLOCKS + 1), (1, -1, 6, 9), (1, 6, -1, 9), (1, 6, 6, -1)):
        assert lib.orbfe_essential_graph_workspace_bytes(*args, C.byref(n)) == inv
    assert lib.orbfe_essential_graph_workspace_bytes(1, 6, 6, 9, None) == inv
    assert lib.orbfe_essential_graph_workspace_bytes(1, _lib.EG_MAX_KEYFRAMES, _lib.EG_MAX_EDGES, _lib.EG_MAX_ENVELOPE_BLOCKS, C.byref(n)) == 0
    one = C.c_void_p(256)
    assert lib.orbfe_essential_graph_batch_device(1, one, one, one, 6, 6, 9, 0, one, one, one, one, 10, None) == inv   # workspace too small
    assert lib.orbfe_essential_graph_batch_device(1, one, one, one, 6, 6, 9, 4, one, one, one, one, 1 << 30, None) == inv   # flags
    assert lib.orbfe_essential_graph_batch_device(1, None, one, one, 6, 6, 9, 0, one, one, one, one, 1 << 30, None) == inv
    assert lib.orbfe_essential_graph_batch_device(1, one, one, one, 6, 6, 9, 0, one, one, one, C.c_void_p(264), 1 << 30, None) == inv
    # the envelope limit: rows that all reach back to the first free vertex
    k = 513
    e = np.zeros(2 * (k - 1), _lib.EG_EDGE_DTYPE)
    e["i"][:k - 1], e["j"][:k - 1] = np.arange(1, k), np.arange(0, k - 1)
    e["i"][k - 1:], e["j"][k - 1:] = np.arange(1, k), 0
    assert optimizer.essential_graph_envelope_blocks(k, None, e) == k * (k + 1) // 2 > _lib.EG_MAX_ENVELOPE_BLOCKS
    W = np.zeros(k, _lib.EG_VERTEX_DTYPE)
    W["Scw"]["q"][:, 3] = W["Snc"]["q"][:, 3] = 1.0
    W["Scw"]["s"] = W["Snc"]["s"] = 1.0
    assert _rc(optimizer.essential_graph, W, e) == inv
    # the map correction
    pts, ref, a, b = correct_points_scene()
    bad = ref.copy()
    bad[5] = 8
    assert _rc(sim3.correct_points, pts, bad, a, b) == inv
    a2 = a.copy()
    a2["s"][1] = 0.0
    assert _rc(sim3.correct_points, pts, ref, a2, b) == inv
    out = np.zeros_like(pts)
    assert lib.orbfe_sim3_correct_points(p(pts), -1, p(ref), p(a), p(b), 8, p(out)) == inv
    assert lib.orbfe_sim3_correct_points(p(pts), _lib.EG_MAX_POINTS + 1, p(ref), p(a), p(b), 8, p(out)) == inv
    assert lib.orbfe_sim3_correct_points(p(pts), 10, None, p(a), p(b), 8, p(out)) == inv
    assert lib.orbfe_sim3_correct_points(p(pts), 10, p(ref), p(a), p(b), _lib.EG_MAX_KEYFRAMES + 1, p(out)) == inv
    assert lib.orbfe_sim3_correct_points_device(one, 10, one, one, 60, one, 8, one, None) == inv          # from_stride
    assert lib.orbfe_sim3_correct_points_device(one, 10, one, one, 64, None, 8, one, None) == inv
