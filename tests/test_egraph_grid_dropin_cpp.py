"""csrc/host/Optimizer_hip.h -- orbfe_host::OptimizeEssentialGraph on a mock map whose pose graph has rows as wide as the map is long
(tests/cpp_egraph_grid): the adapter, compiled with ORBFE_HOST_ESSENTIAL_GRAPH_ACROSS_DEVICE, hands a graph beyond
ORBFE_EG_MAX_ENVELOPE_BLOCKS -- and every graph from the measured crossover kEssentialGraphGridFromBlocks on -- to
orbfe_essential_graph_grid; compiled without it, it refuses such a graph as before.  The routing needs no GPU.  With one: the graph
past the one-workgroup limit is optimised, not refused, and a graph within the limit gives the same SetPose bytes with and without
the macro."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "cpp_egraph_grid")
WITH, WITHOUT = (os.path.join(DIR, "_build", n) for n in ("test_egraph_grid_dropin", "test_egraph_grid_dropin_default"))
PAST = 524                                   # 523 free keyframes, all rows back to the first: 137 026 blocks
WITHIN = (12, 100)                           # 66 blocks, below the crossover, and 4 950, above it


@pytest.fixture(scope="module")
def built():
    _lib.build()
    r = subprocess.run(["make", "-C", DIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return True


def crossover():
    text = open(os.path.join(ROOT, "refactored_orb_slam2_amd", "csrc", "host", "Optimizer_hip.h")).read()
    return int(re.search(r"constexpr int64_t kEssentialGraphGridFromBlocks = (\d+);", text).group(1))


def _exe(exe, tmp_path, n_kf, fix_scale, mode):
    out = tmp_path / f"{os.path.basename(exe)}_{n_kf}_{int(fix_scale)}_{mode}.bin"
    r = subprocess.run([exe, str(n_kf), str(int(fix_scale)), str(out), mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    macro, across, blocks = struct.unpack_from("<iiq", raw, 0)
    calls = poses = None
    if mode == "run":
        rec = np.frombuffer(raw, np.dtype([("calls", "<i4"), ("T", "<f4", (12,))]), n_kf, 16)
        assert 16 + 52 * n_kf == len(raw)
        calls, poses = rec["calls"].copy(), rec["T"].copy()
    return dict(macro=macro, across=across, blocks=blocks, calls=calls, poses=poses, stderr=r.stderr)


def test_the_routing_follows_the_envelope_and_the_named_constant(built, tmp_path):
    x = crossover()
    assert 0 < x <= _lib.EG_MAX_ENVELOPE_BLOCKS
    for n in (PAST,) + WITHIN:
        a, b = _exe(WITH, tmp_path, n, True, "route"), _exe(WITHOUT, tmp_path, n, True, "route")
        assert (a["macro"], b["macro"]) == (1, 0)
        assert a["blocks"] == b["blocks"] == (n - 1) * n // 2
        assert a["across"] == b["across"] == int(a["blocks"] >= x)
    assert (PAST - 1) * PAST // 2 > _lib.EG_MAX_ENVELOPE_BLOCKS >= (WITHIN[1] - 1) * WITHIN[1] // 2


def _gpu():
    import ctypes as C
    n = C.c_int(0)
    return _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [True, False])
def test_a_graph_past_the_one_workgroup_limit_is_optimised_not_refused(built, tmp_path, fix_scale):
    assert _gpu()
    start = _exe(WITHOUT, tmp_path, PAST, fix_scale, "run")
    assert (start["calls"] == 0).all() and "envelope" in start["stderr"]            # refused as before: the map is untouched
    got = _exe(WITH, tmp_path, PAST, fix_scale, "run")
    assert got["blocks"] > _lib.EG_MAX_ENVELOPE_BLOCKS and got["across"] == 1
    assert (got["calls"] == 1).all() and got["stderr"] == ""
    assert got["poses"][0].tobytes() == start["poses"][0].tobytes()                 # the loop keyframe is fixed
    moved = np.abs(got["poses"] - start["poses"]).max(1)
    print(f"past the limit, fix_scale {fix_scale}: {int((moved > 1e-4).sum())} of {PAST} poses moved, the current keyframe's by {moved[-1]:.3f}")
    assert np.isfinite(got["poses"]).all() and moved[-1] > 0.05 and (moved[1:] > 0).all()
    assert moved[1] < moved[-1]                                                     # the correction grows along the trajectory


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("n_kf", WITHIN)
def test_a_graph_within_the_limit_gives_the_same_bytes_either_way(built, tmp_path, n_kf, fix_scale):
    assert _gpu()
    a, b = _exe(WITH, tmp_path, n_kf, fix_scale, "run"), _exe(WITHOUT, tmp_path, n_kf, fix_scale, "run")
    assert (a["calls"] == 1).all() and (b["calls"] == 1).all() and a["stderr"] == b["stderr"] == ""
    assert a["poses"].tobytes() == b["poses"].tobytes()
    print(f"{n_kf} keyframes, {a['blocks']} blocks: across the device {a['across']} with the macro")
    assert a["across"] == int(n_kf == WITHIN[1]), "the smaller graph stays on the one-workgroup form, the larger one compares the two"
