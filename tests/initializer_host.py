"""The host build of csrc/initializer_internal.h (tests/cpp_initializer) behind the same dictionary initializer.initialize returns, for
the CPU suite (against the yardstick) and the GPU suite (against the device, byte for byte)."""
import ctypes as C
import os
import subprocess

import numpy as np

from refactored_orb_slam2_amd import _lib
from refactored_orb_slam2_amd.initializer import bits, init_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_host = None


def host_lib():
    global _host
    if _host is None:
        d = os.path.join(ROOT, "tests", "cpp_initializer")
        r = subprocess.run(["make", "-C", d], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        _host = C.CDLL(os.path.join(d, "_build", "libinitializer_host.so"))
        vp, ci = C.c_void_p, C.c_int
        _host.init_host_run.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
        _host.init_host_decide.argtypes = [ci, vp, vp, ci, vp, vp]
        _host.init_host_first_max.argtypes = [vp, ci]
    return _host


def params_of(p):
    return init_params(*p[:4], sigma=p[4], min_parallax=p[5], min_triangulated=p[6])


def host_run(keys1, keys2, matches12, sets, params) -> dict:
    par = np.ascontiguousarray(params, _lib.INIT_PARAMS_DTYPE).reshape(1)
    k1, k2 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2), np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
    m12, sets = np.ascontiguousarray(matches12, np.int32), np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
    n1, n2, H = len(k1), len(k2), len(sets)
    nw = (n1 + 63) // 64
    result = np.zeros(1, _lib.INIT_RESULT_DTYPE)
    P3D, tri, inl = np.zeros((n1, 3), np.float32), np.zeros(max(nw, 1), np.uint64), np.zeros(max(nw, 1), np.uint64)
    hyps, words, cands = np.zeros((2, H), _lib.INIT_HYPOTHESIS_DTYPE), np.zeros((2, H, nw), np.uint64), np.zeros(8, _lib.INIT_CANDIDATE_DTYPE)
    p = _lib.ptr
    rc = host_lib().init_host_run(p(par), p(k1), n1, p(k2), n2, p(m12), p(sets), H, p(result), p(P3D), p(tri), p(inl), p(hyps), p(words), p(cands))
    assert rc == 0
    N = int(result["n_matches"][0])
    return {"result": result[0], "P3D": P3D, "triangulated": bits(tri, n1), "inliers": bits(inl, N), "hyps_h": hyps[0], "hyps_f": hyps[1],
            "words_h": words[0], "words_f": words[1], "candidates": cands, "triangulated_words": tri[:nw], "inlier_words": inl[:nw]}


def host_decide(model, n_good, parallax, N, params):
    par = np.ascontiguousarray(params, _lib.INIT_PARAMS_DTYPE).reshape(1)
    g, q = np.ascontiguousarray(n_good, np.int32), np.ascontiguousarray(parallax, np.float32)
    result = np.zeros(1, _lib.INIT_RESULT_DTYPE)
    ok = host_lib().init_host_decide(int(model), _lib.ptr(g), _lib.ptr(q), int(N), _lib.ptr(par), _lib.ptr(result))
    return bool(ok), result[0]


def host_first_max(scores):
    s = np.ascontiguousarray(scores, np.float32)
    return int(host_lib().init_host_first_max(_lib.ptr(s), len(s)))
