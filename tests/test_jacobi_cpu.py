"""The Jacobi decompositions and the pose rotation matrix on the CPU: the host build of every user of csrc/jacobi_internal.h and of
pose_rotation (tests/cpp_jacobi/host_arith.cpp) returns the pinned bytes of tests/golden/jacobi_pins.npz, and stays near LAPACK.

Byte pins.  The pins were recorded from the functions as they stood before the arithmetic moved into jacobi_internal.h (tri_null_vector,
ini_svd3, ini_null9_host, sim3_top_eigenvector, pnp_jacobi_serial, pnp_svd_onesided, eg_rotation, pose_to_Tcw) by
tests/golden/make_jacobi_pins.py.  These functions use only + - * / sqrt fabs, so the bytes do not depend on a machine's libm.  Per role:
64 random inputs, the directed cases (zeros, identity, orthogonal columns / diagonal, rank deficient by two with exactly equal smallest
norms, two equal largest eigenvalues, one NaN entry) and the random set scaled by 1e-160 and 1e150 (and 1e-30, 1e30 for float inputs).

Against LAPACK.  On the 64 random inputs of each role, none left out, the largest deviation from numpy's float64 svd / eigh -- a unit
vector up to sign; singular values and U diag(w) Vt for the 3x3; eigenvalues and V diag(d) V^T for the two-sided form; column norms and
W V^T for the one-sided form -- is bounded by twice what the functions showed before the move, plus the final rounding: 2^-24 for
a unit vector's entry rounded to float, 2^-50 (a few ulp of a double entry, for LAPACK builds that differ in the last bits) for the
roles that return doubles.  Measured before the move, and the bound:
    null4   2.944e-08   1.185e-07        two3    3.109e-15   7.105e-15        one62   1.110e-15   3.109e-15
    null9   2.889e-08   1.174e-07        one33   3.192e-15   7.272e-15        one63   7.938e-15   1.676e-14
    eig4    2.959e-08   1.188e-07        one61   3.331e-16   1.554e-15        one64   5.440e-15   1.177e-14
    svd3    8.864e-08   2.369e-07
(svd3 includes the float rounding of singular values up to 2 and of the product.)"""
import os

import numpy as np
import pytest

from tests import jacobi_host as J

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jacobi_pins.npz")
# role -> the deviation from LAPACK measured on the functions before the move (tests/golden/make_jacobi_pins.py prints it)
MEASURED = {"null4": 2.9435820114720457e-08, "null9": 2.8888640146718103e-08, "eig4": 2.958825773280438e-08, "svd3": 8.864477007985982e-08,
            "two3": 3.1086244689504383e-15, "one33": 3.191891195797325e-15, "one61": 3.3306690738754696e-16, "one62": 1.1102230246251565e-15,
            "one63": 7.93809462606987e-15, "one64": 5.440092820663267e-15}
FLOAT_ROLES = ("null4", "null9", "eig4", "svd3")   # their outputs are rounded to float


@pytest.fixture(scope="module")
def pins():
    with np.load(PINS) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def outputs(pins):
    return J.run({k: v for k, v in pins.items() if k.endswith("_in")})


def test_every_role_returns_the_pinned_bytes(pins, outputs):
    assert set(outputs) == {k for k in pins if not k.endswith("_in")}
    for k, got in outputs.items():
        want = pins[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        rows = np.flatnonzero((got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1))
        assert rows.size == 0, f"{k}: inputs {rows.tolist()[:8]} differ from the pin"


def test_the_pins_hold_what_the_header_says(pins):
    n = {k: len(v) for k, v in pins.items() if k.endswith("_in")}
    assert n["null9_in"] == J.N_RANDOM * 3 + 6 and n["null4_in"] == n["svd3_in"] == J.N_RANDOM * 5 + 6
    assert n["eig4_in"] == J.N_RANDOM * 5 + 8 and n["two3_in"] == J.N_RANDOM * 3 + 8 and n["pose_in"] == J.N_RANDOM + 4
    assert all(n[r + "_in"] == J.N_RANDOM * 3 + 6 for r in J.ONESIDED)
    for role, shape in (("null4", (4, 4)), ("null9", (16, 9))):   # the gap of the null-vector roles
        for a in pins[role + "_in"][:J.N_RANDOM]:
            s = np.linalg.svd(a.astype(np.float64).reshape(shape))[1]
            assert np.abs(a).max() <= 1.0 and 10 * s[-1] <= s[-2]
    for role in ("null4", "null9", "svd3", "eig4", "two3", *J.ONESIDED):   # zeros first among the directed cases, one NaN case
        a = pins[role + "_in"]
        assert not a[J.N_RANDOM].any() and sum(int(np.isnan(r).any()) for r in a) == 1
    q = pins["pose_in"][:, :4]
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-15 and (np.abs(q[J.N_RANDOM:]) == 1).sum() == 4


def test_deviation_from_lapack_on_the_random_inputs(pins, outputs):
    errors = J.lapack_errors(pins, outputs)
    assert set(errors) == set(MEASURED)
    for role, err in errors.items():
        bound = 2 * MEASURED[role] + (2.0 ** -24 if role in FLOAT_ROLES else 2.0 ** -50)
        print(f"{role}: deviation {err:.3e}, before the move {MEASURED[role]:.3e}, bound {bound:.3e}")
        assert err <= bound, (role, err, bound)


def test_pose_rotation_is_orthonormal_and_pose_to_Tcw_rounds_it(pins, outputs):
    R, T = outputs["pose_R"].reshape(-1, 3, 3), outputs["pose_T"].reshape(-1, 3, 4)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 4e-15 and np.abs(np.linalg.det(R) - 1).max() < 4e-15
    assert np.array_equal(T[:, :, :3], R.astype(np.float32)) and np.array_equal(T[:, :, 3], pins["pose_in"][:, 4:].astype(np.float32))
    assert np.array_equal(R[J.N_RANDOM], np.eye(3))
    for k in range(3):   # a half turn about axis k
        assert np.array_equal(R[J.N_RANDOM + 1 + k], np.diag([1.0 if i == k else -1.0 for i in range(3)]))
