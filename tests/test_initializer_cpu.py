"""CPU suite of the Initializer: the yardstick of tests/np_initializer.py against itself (R32 inside the non-parity cap per case, the
census of exits), the arithmetic of csrc/initializer_internal.h compiled for the host against the yardstick with the criteria the
GPU suite applies to the device, the selection and acceptance rules on engineered scores and counts, draw_sets against a literal
replay, and the C ABI without a device: struct sizes, exports, every validation boundary on both sides, workspace_bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, initializer
from tests import initializer_host as IH
from tests import np_initializer as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_struct_sizes_and_exports(L):
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for text in ("} orbfe_init_params;", "} orbfe_init_hypothesis;", "} orbfe_init_candidate;", "} orbfe_init_result;", "/* 224 bytes */",
                 f"#define ORBFE_INIT_MAX_MATCHES {_lib.INIT_MAX_MATCHES}", f"#define ORBFE_INIT_MAX_HYPOTHESES {_lib.INIT_MAX_HYPOTHESES}"):
        assert text in hdr, text
    for k, name in enumerate(("FEW_MATCHES", "NO_MODEL", "H_DEGENERATE", "F_FEW_GOOD", "F_SIMILAR", "F_PARALLAX", "H_SECOND", "H_PARALLAX",
                              "H_MIN_TRIANGULATED", "H_FEW_GOOD")):
        assert f"#define ORBFE_INIT_{name} {1 << k} " in hdr and getattr(_lib, "INIT_" + name) == getattr(Y, name) == 1 << k
    for sym in ("orbfe_initializer_initialize", "orbfe_initializer_workspace_bytes", "orbfe_initializer_initialize_batch_device"):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    internal = open(os.path.join(ROOT, "refactored_orb_slam2_amd", "csrc", "initializer_internal.h")).read()
    assert f"#define INI_WAVES {_lib.INIT_WAVES} " in internal
    kernels = open(os.path.join(ROOT, "refactored_orb_slam2_amd", "csrc", "initializer_kernels.hip")).read()
    assert "init_resolve_kernel" not in kernels and "atomicAdd" not in kernels   # no scratch allowance borrowed, no float atomics


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Y.CASES))
def test_yardstick_r32_stays_inside_the_cap(name):
    c = Y.solved(name)
    r64, r32, v = c["r64"], c["r32"], c["v"]
    assert r64["N"] == (45 if name == "few_points" else 300) and len(c["sets"]) == 64
    assert len(c["keys1"]) != len(c["keys2"]) and (c["matches12"] < 0).any()
    print(f"{name}: non-parity share {v['share']:.4f}; model {r64['model']} success {r64['success']} reason {r64['reason']}; "
          f"parity: model {v['model']} winners {v['win_h']} {v['win_f']} acceptance {v['decide']}")
    assert v["share"] <= Y.NON_PARITY_CAP
    for k in ("h", "f"):   # by construction, and stated: on parity decisions single precision alone agrees with the truth
        assert np.array_equal(r64["inl_" + k][v["inl_" + k]], r32["inl_" + k][v["inl_" + k]])
    assert (Y.NULL_GAP, Y.CHI_MARGIN, Y.SCORE_GAP, Y.RH_MARGIN, Y.RT_MARGIN, Y.PARALLAX_MARGIN, Y.D_MARGIN, Y.NON_PARITY_CAP) == \
        (1e-4, 1e-2, 1e-3, 0.02, 1e-2, 0.05, 5e-6, 0.03)


def test_the_scenes_do_what_they_are_named_for():
    r = {n: Y.solved(n)["r64"] for n in Y.CASES}
    assert r["general"]["model"] == 2 and r["general"]["success"]
    assert r["plane_tilted"]["model"] == 1 and r["plane_tilted"]["success"] and r["plane"]["model"] == 1
    assert r["outliers40"]["model"] == 2 and r["outliers40"]["n_inliers"] < 0.7 * 300
    assert r["short_baseline"]["reason"] & Y.H_PARALLAX
    assert r["identical"]["reason"] == Y.H_DEGENERATE
    assert r["forward_similar"]["reason"] & Y.H_SECOND and r["noisy_plane"]["reason"] & Y.F_SIMILAR
    assert r["low_parallax_f"]["reason"] == Y.F_PARALLAX and r["few_points"]["reason"] & Y.H_MIN_TRIANGULATED
    truth = Y.solved("general")["truth"]
    # a sanity bound, not a precision one: the winner is ONE minimal set of eight points with 0.3 px of noise, good to a degree or two
    assert np.abs(r["general"]["R21"] - truth["R"]).max() < 3e-2 and np.abs(r["general"]["t21"] - truth["t"]).max() < 0.2


def test_census_of_exits():
    reached = set()
    for n in Y.CASES:
        reached |= Y.census(Y.solved(n)["r64"])
    print("reached:", sorted(reached))
    assert Y.EXPECTED_CENSUS <= reached, sorted(Y.EXPECTED_CENSUS - reached)


# ---- the host build of initializer_internal.h -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Y.CASES))
def test_host_build_against_the_yardstick(name):
    c = Y.solved(name)
    out = IH.host_run(c["keys1"], c["keys2"], c["matches12"], c["sets"], IH.params_of(c["params"]))
    Y.compare(name, out)
    Y.assert_followed_to_its_exit(name, out)
    if name == "identical":   # every homography of identical lists is the identity: the exit of :590 whichever hypothesis wins
        assert (int(out["result"]["model"]), int(out["result"]["reason"])) == (1, Y.H_DEGENERATE)


def test_host_build_shapes_and_degenerate_sets():
    c = Y.solved("general")
    par = IH.params_of(c["params"])
    full = IH.host_run(c["keys1"], c["keys2"], c["matches12"], c["sets"], par)
    i1 = np.flatnonzero(c["matches12"] >= 0)
    for N in (7, 8, 9, 63, 64, 65, 129):   # the first N matches under sets inside [0, 8): the first N verdicts of those sets' full run
        m = c["matches12"].copy()
        m[i1[N:]] = -1
        sets = np.tile(np.arange(8, dtype=np.int32), (3, 1))
        sets[1] = sets[1][::-1]
        out = IH.host_run(c["keys1"], c["keys2"], m, sets, par)
        ref = IH.host_run(c["keys1"], c["keys2"], c["matches12"], sets, par)
        if N < 8:
            assert int(out["result"]["reason"]) == Y.FEW_MATCHES and int(out["result"]["model"]) == 0
            continue
        for k in ("words_h", "words_f"):
            got, want = initializer.bits(out[k], len(m)), initializer.bits(ref[k], len(m))
            assert np.array_equal(got[:, :N], want[:, :N]) and not got[:, N:].any()
    # a set outside [0, N) or with a repeated index: a zero record, the others untouched
    bad = c["sets"].copy()
    bad[3, 2], bad[5, 7], bad[9, 0] = 300, bad[5, 0], -1
    out = IH.host_run(c["keys1"], c["keys2"], c["matches12"], bad, par)
    for k in ("hyps_h", "hyps_f"):
        keep = np.setdiff1d(np.arange(64), [3, 5, 9])
        assert not out[k][[3, 5, 9]].view(np.uint8).any() and np.array_equal(out[k][keep], full[k][keep])
    assert not out["words_h"][[3, 5, 9]].any() and np.array_equal(out["words_f"][keep], full["words_f"][keep])


def test_selection_rule_on_engineered_scores():
    f = IH.host_first_max
    assert f([]) == -1 and f([0.0, 0.0]) == -1 and f([np.nan, 0.0]) == -1 and f([np.nan, 2.0, np.nan]) == 1
    assert f([1.0, 3.0, 3.0, 2.0]) == 1                                    # the first maximum
    s = np.zeros(200, np.float32)
    s[[70, 6, 134]] = 5.0                                                  # equal maxima in different lanes of the scan: the earliest
    assert f(s) == 6
    s[150] = np.inf
    assert f(s) == 150 and Y.first_max(s) == 150
    rng = np.random.default_rng(0)
    for _ in range(20):
        s = rng.integers(0, 6, 130).astype(np.float32)
        assert f(s) == Y.first_max(s)


def test_acceptance_rules_on_engineered_counts():
    par = initializer.init_params(500, 500, 320, 240)
    d = IH.host_decide
    # ReconstructF (:497-559)
    ok, r = d(2, [100, 3, 0, 2], [2.0, 0, 0, 0], 100, par)
    assert ok and (int(r["best_candidate"]), int(r["n_good"]), int(r["second_good_or_n_similar"])) == (0, 100, 1)
    assert d(2, [89, 3, 0, 2], [2.0, 0, 0, 0], 100, par)[1]["reason"] == Y.F_FEW_GOOD        # nMinGood = max(int(0.9 N), 50) = 90
    assert d(2, [90, 3, 0, 2], [2.0, 0, 0, 0], 100, par)[0]
    assert d(2, [49, 0, 0, 0], [2.0, 0, 0, 0], 40, par)[1]["reason"] == Y.F_FEW_GOOD and d(2, [50, 0, 0, 0], [2.0, 0, 0, 0], 40, par)[0]
    assert d(2, [100, 71, 0, 0], [2.0, 2.0, 0, 0], 100, par)[1]["reason"] == Y.F_SIMILAR     # 71 > 0.7 * 100
    assert d(2, [100, 70, 0, 0], [2.0, 2.0, 0, 0], 100, par)[0]                              # 70 > 70.0 is false
    assert d(2, [100, 3, 0, 2], [1.0, 9, 9, 9], 100, par)[1]["reason"] == Y.F_PARALLAX       # > minParallax, of the FIRST best only
    ok, r = d(2, [5, 100, 100, 0], [0.0, 0.5, 9.0, 0], 100, par)
    assert int(r["reason"]) == Y.F_SIMILAR and int(r["best_candidate"]) == 1
    assert d(2, [80, 80, 0, 0], [2, 2, 0, 0], 100, par)[1]["reason"] == Y.F_FEW_GOOD | Y.F_SIMILAR
    # ReconstructH (:680-720)
    ok, r = d(1, [10, 100, 74, 0, 0, 0, 0, 0], [0, 1.0, 0, 0, 0, 0, 0, 0], 100, par)
    assert ok and (int(r["best_candidate"]), int(r["n_good"]), int(r["second_good_or_n_similar"])) == (1, 100, 74)   # >= minParallax
    assert d(1, [10, 100, 75, 0, 0, 0, 0, 0], [0, 1.0, 0, 0, 0, 0, 0, 0], 100, par)[1]["reason"] == Y.H_SECOND       # 75 < 75.0 is false
    assert d(1, [100, 100, 0, 0, 0, 0, 0, 0], [2.0, 2.0, 0, 0, 0, 0, 0, 0], 100, par)[1]["reason"] == Y.H_SECOND     # an equal count is second
    assert d(1, [0, 100, 0, 0, 0, 0, 0, 0], [0, 0.99, 0, 0, 0, 0, 0, 0], 100, par)[1]["reason"] == Y.H_PARALLAX
    assert d(1, [0, 91, 0, 0, 0, 0, 0, 0], [0, 2.0, 0, 0, 0, 0, 0, 0], 100, par)[0]
    assert d(1, [0, 90, 0, 0, 0, 0, 0, 0], [0, 2.0, 0, 0, 0, 0, 0, 0], 100, par)[1]["reason"] == Y.H_FEW_GOOD        # 90 > 90.0 is false
    assert d(1, [0, 50, 0, 0, 0, 0, 0, 0], [0, 2.0, 0, 0, 0, 0, 0, 0], 40, par)[1]["reason"] == Y.H_MIN_TRIANGULATED
    assert d(1, [0, 51, 0, 0, 0, 0, 0, 0], [0, 2.0, 0, 0, 0, 0, 0, 0], 40, par)[0]
    ok, r = d(1, [0] * 8, [0.0] * 8, 100, par)                                                # bestSolutionIdx stays -1
    assert not ok and int(r["best_candidate"]) == -1
    assert int(r["reason"]) == Y.H_SECOND | Y.H_PARALLAX | Y.H_MIN_TRIANGULATED | Y.H_FEW_GOOD


# ---- draw_sets -----------------------------------------------------------------------------------------------------------------------
def test_draw_sets_against_a_literal_replay():
    state = [12345]

    def rand():   # any deterministic stream; RandomInt(min, max) = min + int(rand() / (RAND_MAX + 1.0) * (max - min + 1))
        state[0] = (state[0] * 1103515245 + 12345) & 0x7fffffff
        return state[0]

    N, H = 37, 25
    got = initializer.draw_sets(N, H, lambda k: int(rand() / (0x7fffffff + 1.0) * k))
    state[0] = 12345
    want = []
    for _ in range(H):   # :80-93, literally
        avail = list(range(N))
        row = []
        for _j in range(8):
            randi = 0 + int(rand() / (0x7fffffff + 1.0) * ((len(avail) - 1) - 0 + 1))
            row.append(avail[randi])
            avail[randi] = avail[-1]
            avail.pop()
        want.append(row)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert all(len(set(r)) == 8 and min(r) >= 0 and max(r) < N for r in got.tolist())
    assert np.array_equal(initializer.draw_sets(20, 5, np.random.default_rng(3)), Y.draw_sets(20, 5, 3))
    with pytest.raises(ValueError):
        initializer.draw_sets(7, 1, np.random.default_rng(0))


# ---- the C ABI without a device ----------------------------------------------------------------------------------------------------
def _init(L, n1=10, n2=12, H=2, null=None, bad_match=None, bad_set=None):
    par = initializer.init_params(500, 500, 320, 240)
    k1, k2 = np.zeros((max(n1, 1), 2), np.float32), np.zeros((max(n2, 1), 2), np.float32)
    m = np.full(max(n1, 1), -1, np.int32)
    k = max(min(n1, n2, 9), 0)
    m[:k] = np.arange(k)
    if bad_match is not None:
        m[0] = bad_match
    sets = np.tile(np.arange(8, dtype=np.int32), (max(H, 1), 1))
    nw = (max(n1, 1) + 63) // 64
    a = {"params": par, "keys1": k1, "keys2": k2, "matches12": m, "sets": sets, "result": np.zeros(1, _lib.INIT_RESULT_DTYPE),
         "P3D": np.zeros((max(n1, 1), 3), np.float32), "tri": np.zeros(nw, np.uint64), "inl": np.zeros(nw, np.uint64)}
    if null:
        a[null] = None
    p = _lib.ptr
    return L.orbfe_initializer_initialize(p(a["params"]), p(a["keys1"]), n1, p(a["keys2"]), n2, p(a["matches12"]), p(a["sets"]), H,
                                          p(a["result"]), p(a["P3D"]), p(a["tri"]), p(a["inl"]), None, None, None, None, None)


def test_initialize_validation(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    M, HM = _lib.INIT_MAX_MATCHES, _lib.INIT_MAX_HYPOTHESES
    assert _init(L) == good
    assert _init(L, n1=-1) == _lib.ERR_INVALID and _init(L, n1=0) == good
    assert _init(L, n1=M) == good and _init(L, n1=M + 1) == _lib.ERR_INVALID
    assert _init(L, n2=-1) == _lib.ERR_INVALID and _init(L, n2=0) == good
    assert _init(L, n2=M) == good and _init(L, n2=M + 1) == _lib.ERR_INVALID
    assert _init(L, H=-1) == _lib.ERR_INVALID and _init(L, H=0) == good
    assert _init(L, H=HM) == good and _init(L, H=HM + 1) == _lib.ERR_INVALID
    assert _init(L, bad_match=12) == _lib.ERR_INVALID and _init(L, bad_match=11) == good    # an index into keys2[12]
    for null in ("params", "keys1", "keys2", "matches12", "sets", "result", "P3D", "tri", "inl"):
        assert _init(L, null=null) == _lib.ERR_INVALID, null
    assert _init(L, H=0, null="sets") == good and _init(L, n2=0, null="keys2") == good


def _batch(L, P=0, cap=8, h_cap=8, null=None, misalign=None, ws=None):
    """Nothing is launched for P == 0, so the pointers only have to look like device pointers."""
    names = ("params", "keys1", "n1", "keys2", "n2", "matches12", "sets", "H", "result", "P3D", "tri", "inl", "hyps", "words", "cands", "ws")
    a = {k: 0x10000 * (i + 1) for i, k in enumerate(names)}
    if null:
        a[null] = 0
    if misalign:
        a[misalign[0]] += misalign[1]
    need = C.c_size_t(0)
    if L.orbfe_initializer_workspace_bytes(max(P, 0) if P <= _lib.INIT_MAX_PROBLEMS else 0, min(max(cap, 1), _lib.INIT_MAX_MATCHES), C.byref(need)):
        need = C.c_size_t(0)
    v = lambda k: C.c_void_p(a[k])
    return L.orbfe_initializer_initialize_batch_device(P, v("params"), v("keys1"), v("n1"), v("keys2"), v("n2"), cap, v("matches12"), v("sets"),
                                                       v("H"), h_cap, v("result"), v("P3D"), v("tri"), v("inl"), v("hyps"), v("words"),
                                                       v("cands"), v("ws"), need.value if ws is None else ws, None)


def test_batch_validation_and_workspace_bytes(L):
    good = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    M, HM, PM = _lib.INIT_MAX_MATCHES, _lib.INIT_MAX_HYPOTHESES, _lib.INIT_MAX_PROBLEMS
    assert _batch(L) == good
    assert _batch(L, P=-1) == _lib.ERR_INVALID and _batch(L, P=PM + 1) == _lib.ERR_INVALID
    assert _batch(L, cap=0) == _lib.ERR_INVALID and _batch(L, cap=1) == good
    assert _batch(L, cap=M) == good and _batch(L, cap=M + 1) == _lib.ERR_INVALID
    assert _batch(L, h_cap=0) == _lib.ERR_INVALID and _batch(L, h_cap=1) == good
    assert _batch(L, h_cap=HM) == good and _batch(L, h_cap=HM + 1) == _lib.ERR_INVALID
    for k in ("params", "keys1", "n1", "keys2", "n2", "matches12", "sets", "H", "result", "P3D", "tri", "inl", "hyps", "words", "cands", "ws"):
        assert _batch(L, null=k) == _lib.ERR_INVALID, k
        assert _batch(L, misalign=(k, 2)) == _lib.ERR_INVALID, k
    for k in ("tri", "inl", "words", "ws"):
        assert _batch(L, misalign=(k, 4)) == _lib.ERR_INVALID, k
    assert _batch(L, misalign=("hyps", 4)) == good
    # the workspace: a header of 160 bytes, 16 bytes and 4 bytes a keypoint, each region rounded up to 256 bytes
    up = lambda b: (b + 255) // 256 * 256
    for P, cap in ((1, 1), (3, 300), (8, 1500), (2, M)):
        assert initializer.workspace_bytes(P, cap) == up(P * 160) + up(P * cap * 16) + up(P * cap * 4)
    assert initializer.workspace_bytes(0, 5) == 0
    n = C.c_size_t(0)
    f = L.orbfe_initializer_workspace_bytes
    assert f(-1, 8, C.byref(n)) == _lib.ERR_INVALID and f(PM + 1, 8, C.byref(n)) == _lib.ERR_INVALID and f(PM, 8, C.byref(n)) == _lib.OK
    assert f(1, 0, C.byref(n)) == _lib.ERR_INVALID and f(1, M + 1, C.byref(n)) == _lib.ERR_INVALID and f(1, M, C.byref(n)) == _lib.OK
    assert f(1, 8, None) == _lib.ERR_INVALID
    need = initializer.workspace_bytes(2, 64)
    assert _batch(L, P=2, cap=64, ws=need - 1) == _lib.ERR_INVALID
    if not _gpu_present(L):
        assert _batch(L, P=2, cap=64, ws=need) == _lib.ERR_NO_DEVICE


def test_no_device_is_an_error_not_a_fallback(L):
    c = Y.solved("general")
    args = (IH.params_of(c["params"]), c["keys1"], c["keys2"], c["matches12"], c["sets"])
    if _gpu_present(L):
        assert int(initializer.initialize(*args)["result"]["n_matches"]) == 300
        return
    with pytest.raises(_lib.OrbfeError) as e:
        initializer.initialize(*args)
    assert e.value.code == _lib.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
