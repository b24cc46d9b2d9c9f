"""csrc/pnp_internal.h compiled for the host (tests/cpp_pnp/host_arith.cpp) behind the shape of pnp.pnp_solve, and the cases of
tests/np_pnp.py built once: what tests/test_pnp_cpu.py, tests/test_pnp_gpu.py and tests/test_pnp_dropin_cpp.py share."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from refactored_orb_slam2_amd import _lib
from refactored_orb_slam2_amd.pnp import PnpSolution
from tests import np_pnp as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "cpp_pnp")


@functools.lru_cache(None)
def host_lib():
    subprocess.run(["make", "-C", DIR, "_build/libpnp_host.so"], check=True, capture_output=True)
    return C.CDLL(os.path.join(DIR, "_build", "libpnp_host.so"))


@functools.lru_cache(None)
def case(name):
    """a case of np_pnp.make_case, built once and shared; nobody writes into it"""
    c = Y.make_case(name)
    c["points"].setflags(write=False)
    c["sets"].setflags(write=False)
    return c


def camera(cam):
    c = np.zeros(1, _lib.PNP_CAMERA_DTYPE)
    for k in ("fx", "fy", "cx", "cy"):
        c[k] = cam[k]
    return c


def host_solve(cam, points, sets, min_inliers) -> PnpSolution:
    """pnp_host_solve: the three launches of orbfe_pnp_solve with one lane doing every item"""
    pts, sets = np.ascontiguousarray(points, _lib.PNP_POINT_DTYPE), np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
    n, H = len(pts), len(sets)
    nw = (n + 63) // 64
    cam = camera(cam)
    hy, rf = np.zeros(H, _lib.PNP_HYPOTHESIS_DTYPE), np.zeros(H, _lib.PNP_REFINE_DTYPE)
    w, rw = np.zeros((H, nw), np.uint64), np.zeros((H, nw), np.uint64)
    dg, rdg = np.zeros(H, _lib.PNP_DIAG_DTYPE), np.zeros(H, _lib.PNP_DIAG_DTYPE)
    res, mask = np.zeros(1, _lib.PNP_RESULT_DTYPE), np.zeros(max(nw, 1), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    host_lib().pnp_host_solve(p(cam), p(pts), n, p(sets), H, int(min_inliers), p(hy), p(w), p(rf), p(rw), p(dg), p(rdg), p(res), p(mask))
    return PnpSolution(res[0], mask[:nw], hy, w, rf, rw, dg, rdg)
