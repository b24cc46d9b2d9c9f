"""Writes tests/golden/jacobi_pins.npz: the inputs of every role of tests/cpp_jacobi/host_arith.cpp and the bytes the host build
returns for them.  The decompositions use only + - * / sqrt fabs, so the bytes do not depend on a machine's libm.  Run from the
repository root with the library's headers in the state whose bytes are to be pinned:

    python -m tests.golden.make_jacobi_pins

It also prints each role's largest deviation from LAPACK on the random inputs, which tests/test_jacobi_cpu.py bounds.

Inputs per role: N_RANDOM random matrices with entries in +-1 (the null-vector roles: the smallest singular value at least ten times
below the next), then the directed cases (all zeros, the identity, columns already orthogonal / a diagonal matrix, rank deficient by
two with exactly equal smallest norms, two equal largest eigenvalues for the 4x4 eigenvector, one NaN entry), then the random set
scaled by 1e-160 and by 1e150, where alpha * beta under- and overflows.  A float role cannot hold those two scales (they round to 0
and to inf, which is pinned too), so it also gets 1e-30 and 1e30."""
import os

import numpy as np

from tests import jacobi_host as J

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jacobi_pins.npz")
B3 = np.array([[2.0, -1.0, 2.0], [2.0, 2.0, -1.0], [-1.0, 2.0, 2.0]]) / 4   # exactly orthogonal columns of norm 3 / 4


def hadamard(n):
    h = np.ones((1, 1))
    while len(h) < n:
        h = np.block([[h, h], [h, -h]])
    return h


def orthogonal_columns(m, k):
    """m x k with exactly orthogonal columns of different norms"""
    if m in (4, 16):
        a = hadamard(m)[:, :k] / 4
    else:
        a = np.zeros((6, 6))
        a[:3, :3] = B3
        a[3:, 3:] = B3
        a = a[:m, :k]
    return a * (0.5 ** np.arange(k))


def with_gap(rng, m, k):
    """entries inside +-1, the smallest singular value at least ten times below the next (checked on the float32 values)"""
    while True:
        u = np.linalg.qr(rng.standard_normal((m, k)))[0]
        v = np.linalg.qr(rng.standard_normal((k, k)))[0]
        s = np.sort(rng.uniform(0.3, 1.0, k))[::-1]
        s[-1] = s[-2] * rng.uniform(0.0, 0.05)
        a = ((u * s) @ v.T).astype(np.float32).astype(np.float64)
        sv = np.linalg.svd(a)[1]
        if np.abs(a).max() <= 1.0 and 10 * sv[-1] <= sv[-2]:
            return a


def matrix_role(rng, m, k, gap, scales):
    rand = [with_gap(rng, m, k) if gap else rng.uniform(-1, 1, (m, k)).astype(np.float32).astype(np.float64) for _ in range(J.N_RANDOM)]
    two_zero = rng.uniform(-1, 1, (m, k)).astype(np.float32).astype(np.float64)
    two_zero[:, [min(1, k - 1), k - 1]] = 0.0          # two zero columns: their norms are exactly equal, the first of them is taken
    doubled = rng.uniform(-1, 1, (m, k)).astype(np.float32).astype(np.float64)
    doubled[:, k - 1] = doubled[:, 0]                  # rank deficient by two through repeated columns
    doubled[:, max(k - 2, 0)] = doubled[:, min(1, k - 1)]
    nan = rand[0].copy()
    nan[m // 2, k // 2] = np.nan
    directed = [np.zeros((m, k)), np.eye(m, k), orthogonal_columns(m, k), two_zero, doubled, nan]
    return np.stack(rand + directed + [a * s for s in scales for a in rand]).reshape(-1, m * k)


def symmetric_role(rng, n, scales):
    def sym(a):
        return (np.triu(a) + np.triu(a, 1).T).astype(np.float32).astype(np.float64)

    def rotated(d):
        q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        return sym(q @ np.diag(d) @ q.T)

    rand = [sym(rng.uniform(-1, 1, (n, n))) for _ in range(J.N_RANDOM)]
    d2 = [1.0, 0.5] + [0.0] * (n - 2)
    top = [0.25, 1.0, 1.0, -0.5][:n]
    nan = rand[0].copy()
    nan[0, n - 1] = nan[n - 1, 0] = np.nan
    directed = [np.zeros((n, n)), np.eye(n), np.diag([0.5, -0.25, 1.0, 0.125][:n]), np.diag(d2[::-1]), rotated(d2), np.diag(top),
                rotated([1.0, 1.0, 0.2, -0.7][:n]), nan]
    return np.stack(rand + directed + [a * s for s in scales for a in rand])


def poses(rng):
    q = rng.standard_normal((J.N_RANDOM, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    p = np.concatenate([q, rng.uniform(-5, 5, (J.N_RANDOM, 3))], axis=1)
    fixed = np.zeros((4, 7))
    fixed[0, 3] = 1.0                     # the identity
    fixed[1, 0] = fixed[2, 1] = fixed[3, 2] = 1.0   # a half turn about x, y, z
    fixed[1:, 4:] = [[1.0, -2.0, 3.0]] * 3
    return np.concatenate([p, fixed])


def make_inputs():
    rng = np.random.default_rng(20241228)
    wide, narrow = (1e-160, 1e150), (1e-160, 1e150, 1e-30, 1e30)
    f32 = np.float32
    with np.errstate(over="ignore"):
        i = {"null4_in": matrix_role(rng, 4, 4, True, narrow).astype(f32), "svd3_in": matrix_role(rng, 3, 3, False, narrow).astype(f32),
             "null9_in": matrix_role(rng, 16, 9, True, wide),
             "eig4_in": np.stack([a[np.triu_indices(4)] for a in symmetric_role(rng, 4, narrow)]).astype(f32),
             "two3_in": symmetric_role(rng, 3, wide).reshape(-1, 9)}
    for role, (m, k) in J.ONESIDED.items():
        i[role + "_in"] = matrix_role(rng, m, k, False, wide)
    i["pose_in"] = poses(rng)
    return i


if __name__ == "__main__":
    inputs = make_inputs()
    outputs = J.run(inputs)
    np.savez_compressed(OUT, **inputs, **outputs)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {sum(len(v) for v in inputs.values())} inputs")
    for role, err in J.lapack_errors(inputs, outputs).items():
        print(f"{role}: {err!r}  (2^{np.log2(err):.2f})")
