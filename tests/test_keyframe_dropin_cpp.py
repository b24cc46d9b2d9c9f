"""The C++ side of the keyframe decision and the close stereo points (tests/cpp_keyframe).

host_arith: csrc/keyframe_internal.h compiled for the host under the address and undefined-behaviour sanitizers, a stand-alone program
that runs the sequential form of the rules over every directed scene of tests/np_keyframe.py -- each frame alone and in a batch of five --
and must leave, byte for byte, what the yardstick's reading leaves.  No GPU is involved and nothing is preloaded.

test_keyframe_dropin: orbfe_host::NeedNewKeyFrame / CreateNewKeyFramePoints / UpdateLastFramePoints / StereoInitializationPoints
(csrc/host/Tracking_hip.h) on mock Frame / KeyFrame / MapPoint / Map / LocalMapping against the four reference bodies restated on the
same mocks, over the same scenes: it builds everywhere and fails loudly without a device (a log line, every object as it was built); on
the GPU object state, creation order, the log of every call the mocks received and the return values are equal."""
import ctypes as C
import os
import subprocess

import pytest

from refactored_orb_slam2_amd import _lib
from tests import np_keyframe as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "cpp_keyframe")
EXE, ARITH = os.path.join(DIR, "_build", "test_keyframe_dropin"), os.path.join(DIR, "_build", "host_arith")


def _build(target):
    _lib.build()
    subprocess.run(["make", "-C", DIR, "_build/" + target], check=True, capture_output=True)


def _gpu_present():
    n = C.c_int(0)
    return _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0


@pytest.fixture(scope="module")
def calls_file(tmp_path_factory):
    calls = M.directed_calls()
    path = str(tmp_path_factory.mktemp("keyframe") / "calls.bin")
    M.export_calls(path, calls)
    return path, calls


def test_host_arithmetic_under_sanitizers_equals_the_yardstick(calls_file, tmp_path):
    if _gpu_present():   # sanitizers stay away from GPUs; the rules are host code and the machines without one check them
        pytest.skip("a GPU is present")
    path, calls = calls_file
    _build("host_arith")
    answers = str(tmp_path / "answers.bin")
    r = subprocess.run([ARITH, path, answers], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(calls)} calls" in r.stdout and len(calls) >= 70
    got, want = open(answers, "rb").read(), M.answers_of(calls)
    assert len(got) == len(want)
    assert got == want


def test_dropin_builds_and_fails_loudly_without_a_device(calls_file):
    _build("test_keyframe_dropin")
    assert os.path.exists(EXE)
    r = subprocess.run([EXE, calls_file[0]], capture_output=True, text=True, timeout=300)
    if _gpu_present():
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return
    assert r.returncode == 3
    assert "orbfe_keyframe_insertion failed" in r.stderr and "no HIP device" in r.stderr
    assert "left every object as it was" in r.stdout


@pytest.mark.gpu
def test_dropin_equals_the_restated_reference_bodies(calls_file):
    _build("test_keyframe_dropin")
    r = subprocess.run([EXE, calls_file[0]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert not [l for l in lines if "DIFFERENT" in l]
    s = lines[-1].split()
    tally = {s[i]: int(s[i + 1]) for i in range(0, len(s), 2)}
    # six frames of each refused case with damaged tables are passed over (real objects cannot express them); the two octave cases
    # are refused by the adapter with every object as it was
    assert tally["frames"] == tally["equal"] and tally["frames"] >= 200 and tally["passed_over"] == 7 * 4 and tally["refused"] == 2 * 4
    assert tally["needs"] > 100 and tally["created"] > 10000
    # the only lines on stderr are those of the refused frames
    assert r.stderr.count("the frame was refused") == tally["refused"] and "failed" not in r.stderr
