"""The region arithmetic of a one-problem host call (HostLayout in csrc/host_internal.h), checked without a device by the stand-alone
program of tests/cpp_hostcall, built with the address and undefined-behaviour sanitizers and run as its own executable."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "cpp_hostcall")


def test_host_layout_offsets_under_sanitizers():
    subprocess.run(["make", "-C", DIR], check=True, capture_output=True)
    r = subprocess.run([os.path.join(DIR, "_build", "test_host_layout")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.strip() == "host layout: ok"
