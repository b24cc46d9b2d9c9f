"""The users of csrc/jacobi_internal.h and pose_rotation compiled for the host (tests/cpp_jacobi/host_arith.cpp) behind numpy arrays,
and the error of each role against LAPACK: what tests/test_jacobi_cpu.py and tests/golden/make_jacobi_pins.py share."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "cpp_jacobi")
N_RANDOM = 64   # the first N_RANDOM inputs of every role are the random set, which is compared with LAPACK
ONESIDED = {"one33": (3, 3), "one61": (6, 1), "one62": (6, 2), "one63": (6, 3), "one64": (6, 4)}   # the shapes PnP calls


@functools.lru_cache(None)
def host_lib():
    subprocess.run(["make", "-C", DIR, "_build/libjacobi_host.so"], check=True, capture_output=True)
    return C.CDLL(os.path.join(DIR, "_build", "libjacobi_host.so"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(inputs):
    """inputs: {role + "_in": array}; returns {role + "_" + output: array} of every role, computed by the host library"""
    h = host_lib()
    f32, f64 = np.float32, np.float64
    o = {}
    a = np.ascontiguousarray(inputs["null4_in"], f32)
    o["null4_v"] = np.zeros((len(a), 4), f32)
    h.jacobi_host_null4(_p(a), len(a), _p(o["null4_v"]))
    a = np.ascontiguousarray(inputs["svd3_in"], f32)
    o["svd3_U"], o["svd3_w"], o["svd3_Vt"] = np.zeros((len(a), 9), f32), np.zeros((len(a), 3), f32), np.zeros((len(a), 9), f32)
    h.jacobi_host_svd3(_p(a), len(a), _p(o["svd3_U"]), _p(o["svd3_w"]), _p(o["svd3_Vt"]))
    a = np.ascontiguousarray(inputs["null9_in"], f64)
    o["null9_v"] = np.zeros((len(a), 9), f32)
    h.jacobi_host_null9(_p(a), len(a), _p(o["null9_v"]))
    a = np.ascontiguousarray(inputs["eig4_in"], f32)
    o["eig4_q"] = np.zeros((len(a), 4), f32)
    h.jacobi_host_eig4(_p(a), len(a), _p(o["eig4_q"]))
    a = np.array(inputs["two3_in"], f64, order="C")   # in place: a copy
    o["two3_A"], o["two3_V"] = a, np.zeros((len(a), 9), f64)
    h.jacobi_host_twosided(_p(a), _p(o["two3_V"]), 3, len(a))
    for role, (m, k) in ONESIDED.items():
        a = np.array(inputs[role + "_in"], f64, order="C")
        o[role + "_W"], o[role + "_V"] = a, np.zeros((len(a), k * k), f64)
        h.jacobi_host_onesided(_p(a), _p(o[role + "_V"]), m, k, len(a))
    a = np.ascontiguousarray(inputs["pose_in"], f64)
    o["pose_R"], o["pose_T"] = np.zeros((len(a), 9), f64), np.zeros((len(a), 12), f32)
    h.jacobi_host_pose_rotation(_p(a), len(a), _p(o["pose_R"]))
    h.jacobi_host_pose_to_Tcw(_p(a), len(a), _p(o["pose_T"]))
    return o


def sym4(n10):
    """the symmetric 4x4 of the upper triangle n00 n01 n02 n03 n11 n12 n13 n22 n23 n33"""
    m = np.zeros((4, 4))
    m[np.triu_indices(4)] = n10
    return m + np.triu(m, 1).T


def _up_to_sign(v, r):
    return min(np.abs(v - r).max(), np.abs(v + r).max())


def lapack_errors(inputs, outputs):
    """role -> the largest deviation from numpy's float64 LAPACK over the N_RANDOM random inputs of the role, none left out"""
    e = {}
    n = N_RANDOM
    e["null4"] = max(_up_to_sign(outputs["null4_v"][i].astype(np.float64), np.linalg.svd(inputs["null4_in"][i].astype(np.float64).reshape(4, 4))[2][3])
                     for i in range(n))
    e["null9"] = max(_up_to_sign(outputs["null9_v"][i].astype(np.float64), np.linalg.svd(inputs["null9_in"][i].reshape(16, 9))[2][8]) for i in range(n))
    e["eig4"] = max(_up_to_sign(outputs["eig4_q"][i].astype(np.float64), np.linalg.eigh(sym4(inputs["eig4_in"][i].astype(np.float64)))[1][:, 3])
                    for i in range(n))
    worst = 0.0
    for i in range(n):   # the 3x3 SVD: the singular values and the product U diag(w) Vt
        U, w, Vt = (outputs["svd3_" + k][i].astype(np.float64) for k in ("U", "w", "Vt"))
        u, s, vt = np.linalg.svd(inputs["svd3_in"][i].astype(np.float64).reshape(3, 3))
        worst = max(worst, np.abs(w - s).max(), np.abs(U.reshape(3, 3) @ np.diag(w) @ Vt.reshape(3, 3) - u @ np.diag(s) @ vt).max())
    e["svd3"] = worst
    worst = 0.0
    for i in range(n):   # the two-sided form: the eigenvalues and the product V diag(d) V^T
        d, V = np.diag(outputs["two3_A"][i].reshape(3, 3)), outputs["two3_V"][i].reshape(3, 3)
        w, q = np.linalg.eigh(inputs["two3_in"][i].reshape(3, 3))
        worst = max(worst, np.abs(np.sort(d) - w).max(), np.abs(V @ np.diag(d) @ V.T - q @ np.diag(w) @ q.T).max())
    e["two3"] = worst
    for role, (m, k) in ONESIDED.items():   # the one-sided form: the singular values (column norms) and the product W V^T
        worst = 0.0
        for i in range(n):
            W, V = outputs[role + "_W"][i].reshape(m, k), outputs[role + "_V"][i].reshape(k, k)
            u, s, vt = np.linalg.svd(inputs[role + "_in"][i].reshape(m, k), full_matrices=False)
            worst = max(worst, np.abs(np.sort(np.linalg.norm(W, axis=0))[::-1] - s).max(), np.abs(W @ V.T - u @ np.diag(s) @ vt).max())
        e[role] = worst
    return e
