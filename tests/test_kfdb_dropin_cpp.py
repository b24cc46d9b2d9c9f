"""csrc/host/KeyFrameDatabase_hip.h -- orbfe_host::KeyFrameDatabase, the class with the public surface of ORB_SLAM2::KeyFrameDatabase --
on the mock KeyFrame / Frame of tests/cpp_kfdb: builds everywhere and fails loudly without a device (a log line per call, empty
vectors); on the GPU a scripted sequence of add, erase, clear, covisibility-graph changes and both kinds of query gives, call by call,
the candidates of the Python mirror, which tests/test_kfdb_gpu.py ties to the reading -- in the polling mode, where the program never
announces a graph change, and in the notified mode."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib
from tests import np_kfdb as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp_kfdb", "_build", "test_kfdb_dropin")


def _build():
    _lib.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp_kfdb")], check=True, capture_output=True)


def _vec(ids, vals):
    ids, vals = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64)
    return struct.pack("<i", len(ids)) + ids.tobytes() + vals.tobytes()


def _script():
    """(n_words, ops): make / add / erase / clear / graph (row of ten ids, connected ids) / reloc / loop"""
    n_words = 3000
    rng, map_ops, kfs = K.make_map(21, 70, 7, n_words)
    ops = [("make", kf["id"], kf["ids"], kf["vals"]) for kf in kfs]
    ops += [("add", kf["id"]) for kf in kfs[:60]]
    ops += [("graph", kf["id"], kf["row"], [i for i in kf["row"] if i >= 0]) for kf in kfs]
    qs = K._reloc_queries(rng, kfs, 8, 7, n_words)
    ops += [("reloc", q["ids"], q["vals"]) for q in qs[:3]]
    ops += [("loop", kfs[k]["id"], 0.02) for k in (62, 65, 69)]                      # keyframes that are not in the database yet
    ops += [("add", kf["id"]) for kf in kfs[60:]]
    ops += [("loop", kfs[k]["id"], 0.02) for k in (62, 30)]                          # ... and keyframes that are
    ops += [("erase", kfs[k]["id"]) for k in (5, 31, 32)] + [("erase", 4242)]
    ops += [("graph", kf["id"], kf["row"][::-1], kf["row"][:3]) for kf in kfs[25:40]]   # -1 first: an empty row; other connected sets
    ops += [("graph", kf["id"], [i for i in kf["row"] if i >= 0][::-1], []) for kf in kfs[40:50]]
    ops += [("reloc", q["ids"], q["vals"]) for q in qs[3:6]] + [("loop", kfs[30]["id"], 0.02), ("loop", kfs[45]["id"], 0.0)]
    ops += [("add", kfs[31]["id"]), ("reloc", qs[4]["ids"], qs[4]["vals"]), ("clear",), ("reloc", qs[4]["ids"], qs[4]["vals"])]
    ops += [("add", kf["id"]) for kf in kfs[20:50]]
    ops += [("reloc", q["ids"], q["vals"]) for q in qs[4:]] + [("loop", kfs[10]["id"], 0.01)]
    return n_words, ops


def _serialise(n_words, ops, notified):
    b = struct.pack("<iii", n_words, int(notified), len(ops))
    for op in ops:
        if op[0] == "make":
            b += struct.pack("<iq", 0, op[1]) + _vec(op[2], op[3])
        elif op[0] in ("add", "erase"):
            b += struct.pack("<iq", 1 if op[0] == "add" else 2, op[1])
        elif op[0] == "clear":
            b += struct.pack("<i", 3)
        elif op[0] == "graph":
            row = (list(op[2]) + [-1] * 10)[:10]
            b += struct.pack("<iq10qi", 4, op[1], *row, len(op[3])) + np.array(op[3], np.int64).tobytes()
        elif op[0] == "reloc":
            b += struct.pack("<i", 5) + _vec(op[1], op[2])
        elif op[0] == "loop":
            b += struct.pack("<iqf", 6, op[1], op[2])
    return b


def _run(tmp_path, n_words, ops, notified):
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(pin, "wb") as f:
        f.write(_serialise(n_words, ops, notified))
    r = subprocess.run([EXE, pin, pout], capture_output=True, text=True)
    raw = open(pout, "rb").read() if os.path.exists(pout) else b""
    out, off = [], 0
    while off < len(raw):
        n, = struct.unpack("<i", raw[off:off + 4])
        out.append(np.frombuffer(raw, np.int64, n, off + 4).tolist())
        off += 4 + 8 * n
    return r, out


def _mirror(n_words, ops):
    """the same calls on the Python mirror; a keyframe's row is its prefix up to the first -1, as the mock's vector is"""
    from refactored_orb_slam2_amd.keyframe_database import KeyFrameDatabase
    db = KeyFrameDatabase(n_words)
    objs, out = {}, []
    for op in ops:
        if op[0] == "make":
            objs[op[1]] = dict(ids=op[2], vals=op[3], row=[], conn=[])
        elif op[0] == "add":
            db.add(op[1], objs[op[1]]["ids"], objs[op[1]]["vals"])
            db.set_covisibles([op[1]], [objs[op[1]]["row"] + [-1]])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "graph":
            row = list(op[2])
            row = row[: row.index(-1)] if -1 in row else row
            objs.setdefault(op[1], dict(ids=[], vals=[], row=[], conn=[])).update(row=row[:10], conn=list(op[3]))
            db.set_covisibles([op[1]], [row[:10] + [-1]])
        elif op[0] == "reloc":
            out.append(db.detect_relocalization_candidates(op[1], op[2]))
        elif op[0] == "loop":
            o = objs[op[1]]
            out.append(db.detect_loop_candidates(o["ids"], o["vals"], op[2], o["conn"]))
    return out


def _gpu_present():
    n = C.c_int(0)
    return _lib.lib().orbfe_device_count(C.byref(n)) == 0 and n.value > 0


def test_dropin_builds_and_fails_loudly_without_a_device(tmp_path):
    _build()
    assert os.path.exists(EXE)
    n_words, ops = _script()
    n_queries = sum(op[0] in ("reloc", "loop") for op in ops)
    r, out = _run(tmp_path, n_words, ops, False)
    assert len(out) == n_queries
    if _gpu_present():
        assert r.returncode == 0, r.stderr[-2000:]
        return
    assert r.returncode == 3 and all(c == [] for c in out)
    assert "orbfe_kfdb_create failed" in r.stderr and "no HIP device" in r.stderr
    assert r.stderr.count("DetectRelocalizationCandidates") + r.stderr.count("DetectLoopCandidates") == n_queries


@pytest.mark.gpu
@pytest.mark.parametrize("notified", [False, True])
def test_dropin_equals_the_mirror_call_by_call(tmp_path, notified):
    _build()
    n_words, ops = _script()
    r, out = _run(tmp_path, n_words, ops, notified)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    want = _mirror(n_words, ops)
    assert len(out) == len(want) == sum(op[0] in ("reloc", "loop") for op in ops)
    for k, (a, b) in enumerate(zip(out, want)):
        assert a == b, k
    assert sum(len(c) > 0 for c in want) >= 12 and sum(len(c) > 1 for c in want) >= 3 and [] in want
