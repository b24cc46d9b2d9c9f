"""What the listing of orient_describe8_kernel must keep (tools/describe_isa.py; needs hipcc, no GPU): the per-keypoint loops fetch their
plane constants with v_readlane -- no scalar load in either of them -- the kernel stays within the register budget of seven waves per
SIMD without scratch memory, and the compiler keeps nothing in M0, which the LDS-DMA statements write without restoring it."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def isa():
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    import describe_isa
    res, body = describe_isa.report()
    return res, body


def test_two_per_keypoint_loops_without_scalar_loads(isa):
    res, _ = isa
    assert len(res["loops"]) == 2, res["loops"]   # phase 1 (moments) and phase 3 (BRIEF)
    for lp in res["loops"]:
        assert lp["s_load"] == 0, lp
        assert lp["lds_dma"] in (2, 3), lp   # a raw window is two load rounds, a blurred one two or three


def test_loops_stay_below_the_parent_listing(isa):
    """The longest way through each loop body, counted by tools/describe_isa.py: 169 and 330 instructions in the kernel this one replaced
    (profiles/r07_describe.md).  The bound asked for here is not the measured figure (100 and 210) but what the rewrite set out to remove
    at the least: 120 instructions per keypoint over both loops."""
    res, _ = isa
    total = sum(lp["longest_path"][0] for lp in res["loops"])
    assert total <= 169 + 330 - 120, res["loops"]


def test_register_budget_and_m0(isa):
    res, body = isa
    assert res["scratch_bytes"] == 0
    assert res["vgprs"] <= 72   # seven waves per SIMD
    assert res["m0_writes_outside_asm"] == []
    # no instruction outside the inline-asm blocks reads M0 either
    in_asm = False
    for line in body.splitlines():
        t = line.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
        elif t.startswith(";;#ASMEND"):
            in_asm = False
        elif not in_asm and not t.startswith(";"):
            assert " m0" not in t.split(";")[0] and ",m0" not in t.split(";")[0], t
