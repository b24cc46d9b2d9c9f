"""csrc/host/Tracking_hip.h -- orbfe_host::UpdateLocalMap -- on the mock Frame / KeyFrame / MapPoint of tests/cpp_localmap: builds
everywhere and fails loudly without a device (a log line, every object as it was built); on the GPU two identical seeded worlds go one
through the adapter and one through Tracking::UpdateLocalKeyFrames, UpdateLocalPoints and the first half of SearchLocalPoints restated on
the same mocks in plain C++, and after every frame both lists, pRefKF, the frame's slots, every mnTrackReferenceForFrame and each local
point's skip are equal."""
import ctypes as C
import os
import subprocess

import pytest

from refactored_orb_slam2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_localmap", "_build", "test_localmap_dropin")


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_localmap"), "_build/test_localmap_dropin"], check=True, capture_output=True)


def _gpu_present():
    n = C.c_int(0)
    return _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_dropin_builds_and_fails_loudly_without_a_device():
    _build()
    assert os.path.exists(EXE)
    r = subprocess.run([EXE, "check", "1"], capture_output=True, text=True, timeout=120)
    if _gpu_present():
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return
    assert r.returncode == 3
    assert "orbfe_covis_count failed" in r.stderr and "no HIP device" in r.stderr
    assert "left every object as it was" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_dropin_equals_the_plain_loops_element_for_element(seed):
    _build()
    r = subprocess.run([EXE, "check", str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-3000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    frames = [l.split() for l in lines if l.startswith("frame")]
    assert len(frames) == 7 and all(f[2] == "EQUAL" for f in frames)
    assert sum(int(f[3]) for f in frames) == 6 and frames[-1][3] == "0"        # the last frame votes for nothing
    assert all(int(f[5]) >= 3 and int(f[7]) >= 50 for f in frames[:-1])          # keyframes and points of a list
    empty, skipped = int(lines[-1].split()[1]), int(lines[-1].split()[3])
    assert empty == 1 and skipped >= 50
