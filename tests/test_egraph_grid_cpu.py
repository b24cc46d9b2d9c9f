"""CPU: the essential-graph optimisation of one graph across the device (orbfe_essential_graph_grid,
orbfe_essential_graph_grid_workspace_bytes, orbfe_essential_graph_grid_device, orbfe_debug_egrid_phases) as far as it can be checked
without one.

(1) The exports, the constants of the header and their mirror in _lib.
(2) Every limit refused one step past its boundary and accepted at it, before a device is looked for; the argument errors of
    tests/test_egraph_cpu.py::test_limits_and_argument_errors for the new entry points; the workspace grows with every cap.
(3) The level plan of the factorisation, which the library computes on the host (orbfe_debug_egrid_level_plan): every block lies above
    every block it reads, and there are at most 2 n_free + 1 levels.
(4) The scene beyond the one-workgroup limit that tests/test_egraph_grid_gpu.py compares with the reading is one on which the reading
    is stable: its dense solve and an envelope solve with a permuted summation order take the same decisions and spread by at most a
    quarter of a unit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from tests import np_egraph as G
from tests.test_egraph_grid_gpu import beyond_limit_reference, beyond_limit_scene, identity_graph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbfe.h")
NAMES = ("orbfe_essential_graph_grid", "orbfe_essential_graph_grid_workspace_bytes", "orbfe_essential_graph_grid_device",
         "orbfe_debug_egrid_phases")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


# ---- (1) exports and constants -----------------------------------------------------------------------------------------------------
def test_exports_and_constants(L):
    text = open(HEADER).read()
    for name, value in (("ORBFE_EGRID_MAX_KEYFRAMES", _lib.EGRID_MAX_KEYFRAMES), ("ORBFE_EGRID_MAX_EDGES", _lib.EGRID_MAX_EDGES),
                        ("ORBFE_EGRID_MAX_ENVELOPE_BLOCKS", _lib.EGRID_MAX_ENVELOPE_BLOCKS)):
        m = re.search(rf"^#define {name} (\d+)$", text, re.M)
        assert m and int(m.group(1)) == value, name
        assert re.search(rf"^ \*   {name} ", text, re.M), f"{name}: no row in the limits table"
    assert (_lib.EGRID_MAX_KEYFRAMES, _lib.EGRID_MAX_EDGES, _lib.EGRID_MAX_ENVELOPE_BLOCKS) == (32768, 262144, 4194304)
    assert (_lib.EGRID_MAX_KEYFRAMES, _lib.EGRID_MAX_EDGES) == (_lib.EG_MAX_KEYFRAMES, _lib.EG_MAX_EDGES)
    for f in NAMES + ("orbfe_debug_egrid_level_plan",):
        assert f in _lib.EXPORTS and getattr(L, f).argtypes and re.search(rf"^int {f}\(", text, re.M), f
    assert "a multi-workgroup form of one problem does not exist" not in text
    assert "SYNCHRONOUS" in text[text.index("ORBFE_EGRID_MAX_KEYFRAMES"):]
    for f in ("essential_graph_grid", "essential_graph_grid_device", "essential_graph_grid_workspace_bytes"):
        assert callable(getattr(optimizer, f)) and f in optimizer.__all__
    assert len(_lib.EGRID_PHASES) == 9
    ms = np.full(len(_lib.EGRID_PHASES), -1.0, np.float32)
    assert L.orbfe_debug_egrid_phases(0, _lib.ptr(ms)) == _lib.OK and (ms == 0).all()     # nothing was timed on this thread


# ---- (2) limits and argument errors ------------------------------------------------------------------------------------------------
def _accepted(L):
    n = C.c_int(0)
    gpu = L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0
    return _lib.OK if gpu else _lib.ERR_NO_DEVICE


def _identity_vertices(n):
    V = np.zeros(n, _lib.EG_VERTEX_DTYPE)
    V["Scw"]["q"][:, 3] = V["Snc"]["q"][:, 3] = 1.0
    V["Scw"]["s"] = V["Snc"]["s"] = 1.0
    if n:
        V["fixed"][0] = 1
    return V


def _host(L, V, E, flags=0, n_kf=None, n_edges=None, null=()):
    so, po = np.zeros(max(len(V), 1), _lib.EG_SIM3_DTYPE), np.zeros((max(len(V), 1), 12), np.float32)
    res = np.zeros(1, _lib.EG_RESULT_DTYPE)
    a = dict(V=_lib.ptr(V) if len(V) else None, E=_lib.ptr(E) if len(E) else None, so=_lib.ptr(so), po=_lib.ptr(po), res=_lib.ptr(res))
    for k in null:
        a[k] = None
    return L.orbfe_essential_graph_grid(a["V"], len(V) if n_kf is None else n_kf, a["E"], len(E) if n_edges is None else n_edges, flags,
                                        a["so"], a["po"], a["res"])


def test_count_limits_at_their_boundary(L):
    """The largest accepted counts pass validation (an identity graph, whose one trial is cheap where a device runs it); one more is
    refused"""
    inv, ok = _lib.ERR_INVALID, _accepted(L)
    K = _lib.EGRID_MAX_KEYFRAMES
    V = _identity_vertices(K)
    none = np.zeros(0, _lib.EG_EDGE_DTYPE)
    assert _host(L, V, none) == ok
    assert _host(L, V, none, n_kf=K + 1) == inv
    E = np.zeros(_lib.EGRID_MAX_EDGES, _lib.EG_EDGE_DTYPE)                    # a chain, walked eight times over
    E["i"] = np.arange(len(E)) % (K - 1) + 1
    E["j"] = E["i"] - 1
    assert _host(L, V, E) == ok
    assert _host(L, V, E, n_edges=len(E) + 1) == inv


def test_envelope_limit_at_its_boundary(L):
    inv, ok = _lib.ERR_INVALID, _accepted(L)
    limit = _lib.EGRID_MAX_ENVELOPE_BLOCKS
    V, E = identity_graph(limit)
    fixed = (V["fixed"] != 0).astype(np.uint8)
    assert optimizer.essential_graph_envelope_blocks(len(V), fixed, E) == limit
    assert _host(L, V, E, _lib.EG_FIX_SCALE) == ok
    V, E = identity_graph(limit + 1)
    assert optimizer.essential_graph_envelope_blocks(len(V), fixed, E) == limit + 1
    assert _host(L, V, E, _lib.EG_FIX_SCALE) == inv
    # what the one-workgroup form refuses passes validation here: 513 rows that all reach back to the first
    k = 513
    e = np.zeros(2 * (k - 1), _lib.EG_EDGE_DTYPE)
    e["i"][:k - 1], e["j"][:k - 1] = np.arange(1, k), np.arange(0, k - 1)
    e["i"][k - 1:], e["j"][k - 1:] = np.arange(1, k), 0
    W = _identity_vertices(k)
    W["fixed"][0] = 0
    assert optimizer.essential_graph_envelope_blocks(k, None, e) == k * (k + 1) // 2 > _lib.EG_MAX_ENVELOPE_BLOCKS
    with pytest.raises(_lib.OrbfeError) as ei:
        optimizer.essential_graph(W, e)
    assert ei.value.code == inv
    n = C.c_size_t(0)
    assert L.orbfe_essential_graph_grid_workspace_bytes(k, len(e), k * (k + 1) // 2, C.byref(n)) == _lib.OK


def _rc(fn, *a):
    with pytest.raises(_lib.OrbfeError) as ei:
        fn(*a)
    return ei.value.code


def test_argument_errors(L):
    """The record rules of tests/test_egraph_cpu.py::test_limits_and_argument_errors, for the new entry points"""
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
        assert _rc(optimizer.essential_graph_grid, W, E) == inv
    W = V.copy()
    W["Scw"]["q"][3] = 0.0
    assert _rc(optimizer.essential_graph_grid, W, E) == inv                    # a quaternion of norm 0
    for i, j, kind in ((6, 0, 0), (-1, 0, 0), (0, 6, 0), (2, 2, 0), (1, 0, 2)):
        F = E.copy()
        F[1] = (i, j, kind)
        assert _rc(optimizer.essential_graph_grid, V, F) == inv
    assert _host(L, V, E, flags=2) == inv                                      # unknown flag
    assert _host(L, V, E, n_kf=-1) == inv and _host(L, V, E, n_edges=-1) == inv
    for null in ("V", "E", "so", "po", "res"):
        assert _host(L, V, E, null=(null,)) == inv, null
    assert _host(L, V, E) == _accepted(L)
    # the SE3 path: a record and a derived measurement beyond |s - 1| <= 1e-3
    s3 = G.case_scene("chain6_se3")
    W = s3["vertices"].copy()
    W["Scw"]["s"][3] = 1 + 2e-3
    assert _rc(optimizer.essential_graph_grid, W, s3["edges"], True) == inv
    W = s3["vertices"].copy()
    W["Snc"]["s"][2], W["Snc"]["s"][3] = 1 + 8e-4, 1 - 8e-4                    # each within the tolerance, their quotient not
    assert _rc(optimizer.essential_graph_grid, W, s3["edges"], True) == inv
    # the device form: counts, flags, pointers, alignment, the workspace
    one, n = C.c_void_p(256), C.c_size_t(0)
    dev = L.orbfe_essential_graph_grid_device
    big = 1 << 30
    need = optimizer.essential_graph_grid_workspace_bytes(6, 6, 0)
    assert dev(one, 6, one, 6, 0, one, one, one, one, need - 1, None) == inv                # workspace too small
    assert dev(one, 6, one, 6, 0, one, one, one, C.c_void_p(264), big, None) == inv         # workspace misaligned
    assert dev(one, 6, one, 6, 0, one, one, one, None, big, None) == inv
    assert dev(one, 6, one, 6, 4, one, one, one, one, big, None) == inv                     # flags
    assert dev(one, -1, one, 6, 0, one, one, one, one, big, None) == inv
    assert dev(one, 6, one, -1, 0, one, one, one, one, big, None) == inv
    assert dev(one, _lib.EGRID_MAX_KEYFRAMES + 1, one, 6, 0, one, one, one, one, 1 << 40, None) == inv
    assert dev(one, 6, one, _lib.EGRID_MAX_EDGES + 1, 0, one, one, one, one, 1 << 40, None) == inv
    assert dev(None, 6, one, 6, 0, one, one, one, one, big, None) == inv
    assert dev(one, 6, None, 6, 0, one, one, one, one, big, None) == inv
    assert dev(one, 6, one, 6, 0, None, one, one, one, big, None) == inv
    assert dev(one, 6, one, 6, 0, one, None, one, one, big, None) == inv
    assert dev(one, 6, one, 6, 0, one, one, None, one, big, None) == inv
    assert dev(C.c_void_p(260), 6, one, 6, 0, one, one, one, one, big, None) == inv         # vertices: 8-byte aligned
    assert dev(one, 6, one, 6, 0, one, one, C.c_void_p(260), one, big, None) == inv         # result: 8-byte aligned
    # workspace bytes
    wb = L.orbfe_essential_graph_grid_workspace_bytes
    for args in ((_lib.EGRID_MAX_KEYFRAMES + 1, 6, 9), (6, _lib.EGRID_MAX_EDGES + 1, 9), (6, 6, _lib.EGRID_MAX_ENVELOPE_BLOCKS + 1),
                 (-1, 6, 9), (6, -1, 9), (6, 6, -1)):
        assert wb(*args, C.byref(n)) == inv, args
    assert wb(6, 6, 9, None) == inv
    assert wb(_lib.EGRID_MAX_KEYFRAMES, _lib.EGRID_MAX_EDGES, _lib.EGRID_MAX_ENVELOPE_BLOCKS, C.byref(n)) == _lib.OK
    assert n.value > _lib.EGRID_MAX_ENVELOPE_BLOCKS * 49 * 8
    assert wb(0, 0, 0, C.byref(n)) == _lib.OK


def test_workspace_bytes_grow_with_every_cap():
    f = optimizer.essential_graph_grid_workspace_bytes
    base = (300, 2500, 9000)
    for i in range(3):
        prev = None
        for v in (0, 1, 7, 64, 1000, 32768):
            caps = list(base)
            caps[i] = v
            b = f(*caps)
            assert b % 256 == 0 and (prev is None or b >= prev), (i, v)
            prev = b
        lo, hi = list(base), list(base)
        lo[i], hi[i] = 64, 32768
        assert f(*hi) > f(*lo), i
    # it holds what the one-workgroup form's workspace holds
    assert f(*base) > optimizer.essential_graph_workspace_bytes(1, *base)


# ---- (3) the level plan ------------------------------------------------------------------------------------------------------------
def _check_plan(L, first):
    nf = len(first)
    first = np.ascontiguousarray(first, np.int32)
    off = np.concatenate([[0], np.cumsum(np.arange(nf) - first + 1)]).astype(np.int64)
    lev = np.zeros(max(int(off[-1]), 1), np.int32)
    n_levels = C.c_int32(-1)
    assert L.orbfe_debug_egrid_level_plan(_lib.ptr(first) if nf else None, nf, _lib.ptr(lev) if nf else None, C.byref(n_levels)) == _lib.OK
    lev = lev[:int(off[-1])]
    at = lambda r, c: int(lev[off[r] + c - first[r]])
    for r in range(nf):
        for c in range(first[r], r + 1):
            reads = [at(r, k) for k in range(first[r], c)]                 # row r's blocks before c
            if c < r:
                reads += [at(c, k) for k in range(max(first[r], first[c]), c + 1)]      # row c from where the two rows overlap, L_cc included
            assert at(r, c) >= 1 and all(at(r, c) > x for x in reads), (r, c)
            assert at(r, c) == 1 + max(reads, default=0), (r, c)           # and no later than it has to be
    assert n_levels.value == (int(lev.max()) if nf else 0)
    assert n_levels.value <= 2 * nf + 1
    assert set(lev.tolist()) == set(range(1, n_levels.value + 1))         # no level is empty
    return n_levels.value


@pytest.mark.parametrize("name", list(G.CASES))
def test_level_plan_of_the_cases(L, name):
    s = G.case_scene(name)
    _, first, blocks = G.envelope(len(s["vertices"]), s["vertices"]["fixed"] != 0, s["edges"])
    levels = _check_plan(L, first)
    print(f"{name}: n_free {len(first)}, blocks {blocks}, levels {levels}")


def test_level_plan_of_random_graphs(L):
    rng = np.random.default_rng(7)
    for _ in range(40):
        n = int(rng.integers(2, 30))
        m = int(rng.integers(0, 60))
        e = np.zeros(m, _lib.EG_EDGE_DTYPE)
        e["i"] = rng.integers(0, n, m)
        e["j"] = (e["i"] + rng.integers(1, n, m)) % n
        fixed = rng.uniform(size=n) < 0.2
        _check_plan(L, G.envelope(n, fixed, e)[1])
    one = C.c_int32(0)
    bad = np.array([0, 2], np.int32)                                      # first[1] > 1
    lev = np.zeros(4, np.int32)
    assert L.orbfe_debug_egrid_level_plan(_lib.ptr(bad), 2, _lib.ptr(lev), C.byref(one)) == _lib.ERR_INVALID
    assert L.orbfe_debug_egrid_level_plan(_lib.ptr(bad), -1, _lib.ptr(lev), C.byref(one)) == _lib.ERR_INVALID


# ---- (4) the scene beyond the one-workgroup limit ----------------------------------------------------------------------------------
def test_stability_of_the_scene_beyond_the_limit():
    """Measured: both runs 3 iterations and 12 trials, spread 0.002 units.  The dense run takes 6 s, the envelope run 25 s"""
    s = beyond_limit_scene(True)
    a, b = beyond_limit_reference(), G.run_case(s, order_seed=11)
    spread = max(G.sim3_units(b["sim3"], a["sim3"]), G.pose_units(b["poses"], a["poses"]))
    print(f"beyond the limit: n_free {a['n_free']}, envelope {a['envelope_blocks']}, iterations {a['iterations']}, trials {a['trials']}, "
          f"min |rho| {min(a['min_rho'], b['min_rho']):.3g}, spread {spread:.3g} units")
    assert a["n_free"] == 523 and a["envelope_blocks"] == 137026 > _lib.EG_MAX_ENVELOPE_BLOCKS
    assert a["decisions"] == b["decisions"] and a["iterations"] == b["iterations"] and a["status"] == b["status"] == 0
    assert a["chi2_last"] < a["chi2_first"]
    assert spread <= G.BOUND_UNITS[True] / 4
