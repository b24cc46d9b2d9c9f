"""GPU: orbfe_essential_graph_grid / orbfe_essential_graph_grid_device -- Optimizer::OptimizeEssentialGraph of ONE graph across the
whole device (csrc/egraph_grid_kernels.hip).

Two criteria.  For a graph the one-workgroup form takes, the BYTES of orbfe_essential_graph: records, poses and the whole result
record, on both paths -- every sum keeps its owner and its order.  For a graph beyond ORBFE_EG_MAX_ENVELOPE_BLOCKS, the numpy reading
of tests/np_egraph.py within np_egraph.BOUND_UNITS of the library's parity criterion, as tests/test_egraph_gpu.py compares the
one-workgroup form; tests/test_egraph_grid_cpu.py shows that the reading is stable on that scene.  Iterations and trials of the large
scenes are printed, not compared.  Every figure is printed before it is asserted."""
import functools
import time

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, optimizer
from refactored_orb_slam2_amd._lib import EG_EDGE_DTYPE, EG_RESULT_DTYPE, EG_SIM3_DTYPE, EG_VERTEX_DTYPE
from tests import np_egraph as G

pytestmark = pytest.mark.gpu


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. every case, both forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CASES))
def test_grid_form_gives_the_bytes_of_the_one_workgroup_form(name):
    s = G.case_scene(name)
    one = optimizer.essential_graph(s["vertices"], s["edges"], s["fix_scale"])
    grid = optimizer.essential_graph_grid(s["vertices"], s["edges"], s["fix_scale"])
    res = grid[2]
    print(f"egrid {name}: status {int(res['status'])}, iterations {int(res['iterations'])}, trials {int(res['trials'])}, n_free "
          f"{int(res['n_free'])}, envelope {int(res['envelope_blocks'])}, chi2 {float(res['chi2_first']):.6g} -> "
          f"{float(res['chi2_last']):.6g}, lambda {float(res['lambda']):.3g}; one workgroup: iterations {int(one[2]['iterations'])}, trials "
          f"{int(one[2]['trials'])}")
    assert grid[2].tobytes() == one[2].tobytes(), (name, grid[2], one[2])
    assert grid[0].tobytes() == one[0].tobytes() and grid[1].tobytes() == one[1].tobytes(), name
    if name in ("edges_0", "no_free", "n_kf_1"):
        assert int(res["iterations"]) == 0 and grid[0].tobytes() == np.ascontiguousarray(s["vertices"]["Scw"]).tobytes()
    if name == "rejected_step_se3":                                        # push / pop
        assert (int(res["iterations"]), int(res["trials"])) == (2, 11)
    if name == "wide":
        assert len(s["vertices"]) == 300 and int(res["iterations"]) >= 1


# ---- 2. the device form -------------------------------------------------------------------------------------------------------------
def _device(V, E, fix_scale, blocks, runs=2):
    """The device form on a workspace filled with 0xCD, `runs` times on the same buffers.  Returns (sim3_out, poses_out, result) of
    every run and whether the inputs are unmodified"""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    d_V, d_E = up(V.view(np.uint8).reshape(-1, 136)), up(E.view(np.uint8).reshape(-1, 12))
    sim3_out = torch.full((len(V), 8), 777.0, dtype=torch.float64, device="cuda")
    poses_out = torch.full((len(V), 12), 777.0, dtype=torch.float32, device="cuda")
    result = torch.zeros(48, dtype=torch.uint8, device="cuda")
    ws = torch.full((optimizer.essential_graph_grid_workspace_bytes(len(V), len(E), blocks),), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    outs = []
    for _ in range(runs):
        with torch.cuda.stream(st):
            optimizer.essential_graph_grid_device(d_V, d_E, sim3_out, poses_out, result, ws, fix_scale=fix_scale, stream=st)
        outs.append((sim3_out.cpu().numpy().copy().view(EG_SIM3_DTYPE).reshape(-1), poses_out.cpu().numpy(),
                     result.cpu().numpy().view(EG_RESULT_DTYPE)[0]))
    same = d_V.cpu().numpy().tobytes() == V.tobytes() and d_E.cpu().numpy().tobytes() == E.tobytes()
    return outs, same


@pytest.mark.parametrize("name", ["band", "band_se3", "rejected_step_se3"])
def test_device_form_gives_the_bytes_of_the_host_form(name):
    s = G.case_scene(name)
    V, E, fs = s["vertices"], s["edges"], s["fix_scale"]
    blocks = G.envelope(len(V), V["fixed"] != 0, E)[2]
    host = optimizer.essential_graph_grid(V, E, fs)
    outs, unmodified = _device(V, E, fs, blocks)
    assert unmodified, "inputs were modified"
    assert same_bytes(outs[0], outs[1]), "a second run on the same buffers differs"
    assert same_bytes(outs[0], host)


@pytest.mark.parametrize("fix_scale", [False, True])
def test_device_form_refuses_what_only_the_device_sees(fix_scale):
    """A NaN in a record; with a fixed scale a derived measurement beyond the tolerance; a workspace that holds one block less than
    the envelope: ORBFE_EG_REFUSED, Scw and its pose written through"""
    s = G.case_scene("chain6_se3" if fix_scale else "chain6")
    E = s["edges"]
    blocks = G.envelope(len(s["vertices"]), s["vertices"]["fixed"] != 0, E)[2]
    bad = [s["vertices"].copy()]
    bad[0]["Snc"]["t"][3, 1] = np.nan
    if fix_scale:
        bad.append(s["vertices"].copy())
        bad[1]["Snc"]["s"][2], bad[1]["Snc"]["s"][3] = 1 + 8e-4, 1 - 8e-4     # only the derived measurement is beyond
    for V in bad:
        (so, po, res), = _device(V, E, fix_scale, blocks, runs=1)[0]
        assert int(res["status"]) == _lib.EG_REFUSED and int(res["iterations"]) == 0 and int(res["n_edges"]) == len(E)
        assert so.tobytes() == np.ascontiguousarray(V["Scw"]).tobytes()
        assert np.array_equal(po, G.poses_of(V["Scw"], fix_scale))
    b = G.case_scene("band_se3" if fix_scale else "band")
    need = G.envelope(len(b["vertices"]), b["vertices"]["fixed"] != 0, b["edges"])[2]
    small = next(n for n in range(need - 1, -1, -1)
                 if optimizer.essential_graph_grid_workspace_bytes(len(b["vertices"]), len(b["edges"]), n) <
                 optimizer.essential_graph_grid_workspace_bytes(len(b["vertices"]), len(b["edges"]), need))
    (so, po, res), = _device(b["vertices"], b["edges"], fix_scale, small, runs=1)[0]
    assert int(res["status"]) == _lib.EG_REFUSED and int(res["envelope_blocks"]) == need
    assert so.tobytes() == np.ascontiguousarray(b["vertices"]["Scw"]).tobytes()


# ---- 3. a failed factorisation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_failed_factorisation(K, fix_scale):
    """K identity vertices, none fixed, chained: H is singular (a gauge freedom) and lambda = 1e-16 vanishes beside its entries, so
    a pivot is not > 0.  The reading: FACTOR_FAILED, 1 iteration, 2 trials, chi2 0"""
    V = np.zeros(K, EG_VERTEX_DTYPE)
    V["Scw"]["q"][:, 3] = V["Snc"]["q"][:, 3] = 1.0
    V["Scw"]["s"] = V["Snc"]["s"] = 1.0
    E = np.zeros(K - 1, EG_EDGE_DTYPE)
    E["i"], E["j"] = np.arange(1, K), np.arange(0, K - 1)
    ref = G.essential_graph(V, E, fix_scale)
    assert (ref["status"], ref["iterations"], ref["trials"], ref["chi2_first"], ref["chi2_last"]) == (1, 1, 2, 0.0, 0.0)
    one = optimizer.essential_graph(V, E, fix_scale)
    grid = optimizer.essential_graph_grid(V, E, fix_scale)
    res = grid[2]
    print(f"egrid failed factorisation K {K} fix_scale {fix_scale}: status {int(res['status'])}, iterations {int(res['iterations'])}, "
          f"trials {int(res['trials'])}, lambda {float(res['lambda']):.3g}")
    assert same_bytes(grid, one)
    assert int(res["status"]) == _lib.EG_FACTOR_FAILED
    assert (int(res["iterations"]), int(res["trials"]), float(res["chi2_first"]), float(res["chi2_last"])) == (1, 2, 0.0, 0.0)


# ---- 4., 5. beyond the one-workgroup limit ------------------------------------------------------------------------------------------
def beyond_limit_scene(fix_scale):
    """523 free vertices whose rows all reach back to the first: 137 026 envelope blocks"""
    return G.make_scene(1, n_kf=524, band=1, n_corrected=2, loop_rows=tuple(range(3, 524)), fix_scale=fix_scale)


@functools.lru_cache(maxsize=None)
def beyond_limit_reference():
    return G.run_case(beyond_limit_scene(True), solve="dense")


def test_beyond_the_one_workgroup_limit_against_the_reading():
    s = beyond_limit_scene(True)
    V, E = s["vertices"], s["edges"]
    assert G.envelope(len(V), V["fixed"] != 0, E)[2] == 137026 > _lib.EG_MAX_ENVELOPE_BLOCKS
    with pytest.raises(_lib.OrbfeError) as ei:
        optimizer.essential_graph(V, E, True)
    assert ei.value.code == _lib.ERR_INVALID
    t0 = time.perf_counter()
    so, po, res = optimizer.essential_graph_grid(V, E, True)
    dt = time.perf_counter() - t0
    ref = beyond_limit_reference()
    us, up = G.sim3_units(so, ref["sim3"]), G.pose_units(po, ref["poses"])
    print(f"egrid beyond the limit (SE3): {dt * 1e3:.0f} ms, records {us:.4g} units, poses {up:.4g} units (bound {G.BOUND_UNITS[True]}), "
          f"iterations {int(res['iterations'])} (reading {ref['iterations']}), trials {int(res['trials'])} (reading {ref['trials']}), chi2 "
          f"{float(res['chi2_first']):.9g} -> {float(res['chi2_last']):.6g} (reading {ref['chi2_first']:.9g} -> {ref['chi2_last']:.6g})")
    assert int(res["n_free"]) == ref["n_free"] == 523 and int(res["envelope_blocks"]) == ref["envelope_blocks"] == 137026
    assert int(res["status"]) == ref["status"] == _lib.EG_DONE
    assert abs(float(res["chi2_first"]) - ref["chi2_first"]) <= 1e-9 * max(1.0, ref["chi2_first"])
    fixed = np.flatnonzero(V["fixed"])
    assert len(fixed) == 1 and so[fixed].tobytes() == np.ascontiguousarray(V["Scw"][fixed]).tobytes()
    assert us <= G.BOUND_UNITS[True] and up <= G.BOUND_UNITS[True], (us, up)


def test_beyond_the_one_workgroup_limit_on_the_sim3_path():
    """The same geometry without a fixed scale.  The reading is too slow to run there"""
    s = beyond_limit_scene(False)
    V, E = s["vertices"], s["edges"]
    t0 = time.perf_counter()
    a = optimizer.essential_graph_grid(V, E, False)
    dt = time.perf_counter() - t0
    b = optimizer.essential_graph_grid(V, E, False)
    res = a[2]
    print(f"egrid beyond the limit (Sim3): {dt * 1e3:.0f} ms, status {int(res['status'])}, iterations {int(res['iterations'])}, trials "
          f"{int(res['trials'])}, chi2 {float(res['chi2_first']):.6g} -> {float(res['chi2_last']):.6g}, envelope {int(res['envelope_blocks'])}")
    assert int(res["status"]) == _lib.EG_DONE and float(res["chi2_last"]) < float(res["chi2_first"])
    assert int(res["n_free"]) == 523 and int(res["envelope_blocks"]) == 137026
    fixed = np.flatnonzero(V["fixed"])
    assert len(fixed) == 1 and a[0][fixed].tobytes() == np.ascontiguousarray(V["Scw"][fixed]).tobytes()
    assert same_bytes(a, b), "a second run differs"


# ---- 6. at the new envelope limit ---------------------------------------------------------------------------------------------------
def identity_graph(target, K=30000):
    """tests/test_egraph_gpu._identity_graph with a chain of K: a fixed vertex 0, a chain of K free vertices behind it and, from the
    end, rows that reach back far enough for the row envelope to have exactly `target` blocks.  Every record is the identity, so the
    error is exactly zero and one trial ends the optimisation: b = 0 and x = 0 whatever the factor holds, so this pins the addressing
    of the envelope -- 64-bit element offsets -- and positive pivots at the limit, NOT the factor's values there.  K = 30 000, so that
    few wide rows meet each other: a wide row's blocks are cheap where the rows it reaches over are narrow."""
    E = [(k, k - 1) for k in range(1, K + 1)]
    remaining = target - (2 * K - 1)
    r = K - 1                                                            # row block r is vertex r + 1
    while remaining > 0:
        add = min(remaining, r - 1)
        E.append((r + 1, r - add))                                       # reaches row block r - 1 - add: add blocks more than the chain's 2
        remaining -= add
        r -= 1
    e = np.zeros(len(E), EG_EDGE_DTYPE)
    e["i"], e["j"] = np.array(E).T
    V = np.zeros(K + 1, EG_VERTEX_DTYPE)
    V["Scw"]["q"][:, 3] = V["Snc"]["q"][:, 3] = 1.0
    V["Scw"]["s"] = V["Snc"]["s"] = 1.0
    V["fixed"][0] = 1
    return V, e


def test_largest_envelope_and_one_block_beyond():
    limit = _lib.EGRID_MAX_ENVELOPE_BLOCKS
    V, e = identity_graph(limit)
    fixed = (V["fixed"] != 0).astype(np.uint8)
    assert optimizer.essential_graph_envelope_blocks(len(V), fixed, e) == limit
    t0 = time.perf_counter()
    sim3_out, poses, res = optimizer.essential_graph_grid(V, e, True)
    dt = time.perf_counter() - t0
    print(f"egrid at the envelope limit: {dt:.2f} s, status {int(res['status'])}, iterations {int(res['iterations'])}, trials "
          f"{int(res['trials'])}, envelope {int(res['envelope_blocks'])}, chi2 {float(res['chi2_first'])}")
    assert int(res["status"]) == _lib.EG_DONE and int(res["envelope_blocks"]) == limit
    assert int(res["iterations"]) == 1 and int(res["trials"]) == 1 and float(res["chi2_first"]) == 0.0
    assert G.sim3_units(sim3_out, V["Scw"]) <= 1.0 and G.pose_units(poses, G.poses_of(V["Scw"], True)) <= 1.0
    V, e = identity_graph(limit + 1)
    assert optimizer.essential_graph_envelope_blocks(len(V), fixed, e) == limit + 1
    with pytest.raises(_lib.OrbfeError) as ei:
        optimizer.essential_graph_grid(V, e, True)
    assert ei.value.code == _lib.ERR_INVALID
