"""examples/mono_kitti.py --initialize --map on a synthetic sequence in the KITTI layout (the tilted plane of
tests/test_initializer_example_gpu.py, which initialises from H): a successful initialisation is followed by the initial map; what
the driver reports and dumps equals orbfe_create_initial_map on the dumped frames, and without --map the dump is what it was."""
import os
import subprocess
import sys

import numpy as np
import pytest

from refactored_orb_slam2_amd import ORBextractor, _lib, initializer, optimizer, synth
from tests.test_initializer_example_gpu import _plane_frame, _write_png_gray

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mono_driver_creates_the_initial_map(tmp_path):
    seq = tmp_path / "01"
    (seq / "image_0").mkdir(parents=True)
    W, H, NF = 1241, 376, 1000
    texture = synth.sequence(W, H, 1, seq=33)[0]
    fracs = [0.0, 1 / 3, 2 / 3, 1.0]
    with open(seq / "times.txt", "w") as f:
        for i, fr in enumerate(fracs):
            _write_png_gray(seq / "image_0" / f"{i:06d}.png", texture if fr == 0 else _plane_frame(texture, fr))
            f.write(f"{i * 0.1:e}\n")
    runs = []
    for flag in ([], ["--map"]):
        dump = str(tmp_path / f"plane{len(flag)}.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mono_kitti.py"), str(seq), "--features", str(NF), "--dump", dump,
                            "--initialize", "--iterations", "64"] + flag, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
        runs.append((np.load(dump), r.stdout))
    (plain, out0), (g, out) = runs
    assert "initial map" not in out0 and not [k for k in plain.files if k.startswith("map_")]
    for k in plain.files:                          # --map adds to the dump and changes nothing that was there
        assert np.array_equal(plain[k], g[k]), k
    ex = ORBextractor(2 * NF, device=0)
    cam = optimizer.pose_camera(718.856, 718.856, 607.1928, 185.2157, 0.0, ex.GetInverseScaleSigmaSquares())
    ex.close()
    par = initializer.init_params(718.856, 718.856, 607.1928, 185.2157)
    xy = lambda k: np.stack([k["x"], k["y"]], 1).astype(np.float32)
    ref, n_maps, n_init = None, 0, 0
    for i in range(len(fracs)):
        state = str(g[f"state_{i}"])
        if state == "reference":
            ref = g[f"kp_{i}"]
        if state != "initialized":
            assert f"map_{i}" not in g.files
            continue
        n_init += 1
        cur = g[f"kp_{i}"]
        ini = initializer.initialize(par, xy(ref), xy(cur), g[f"m12_{i}"], g[f"sets_{i}"])
        assert ini["result"].tobytes() == g[f"init_{i}"].tobytes()
        made = initializer.create_initial_map(cam, xy(ref), xy(cur), g[f"m12_{i}"], ini["P3D"], ini["triangulated_words"], ini["result"],
                                              ref["octave"], cur["octave"])
        mr = g[f"map_{i}"]
        assert mr.dtype == _lib.INITIAL_MAP_RESULT_DTYPE and mr.tobytes() == made["result"].tobytes()
        assert g[f"map_poses_{i}"].tobytes() == made["poses"].tobytes() and g[f"map_points_{i}"].tobytes() == made["points"].tobytes()
        assert np.array_equal(g[f"map_index_{i}"], made["index"])
        print(f"frame {i}: {int(mr['n_points'])} points, median depth {float(mr['median_depth']):.4f}, chi2 {float(mr['ba']['chi2_first']):.1f} -> "
              f"{float(mr['ba']['chi2_final']):.1f}, success {int(mr['success'])}, reason {int(mr['reason'])}")
        assert int(mr["n_points"]) == int(ini["result"]["n_triangulated"]) and int(mr["ba"]["rounds"]) == 1
        assert float(mr["ba"]["chi2_final"]) <= float(mr["ba"]["chi2_first"])
        assert f"frame {i}: initial map of {int(mr['n_points'])} points, median depth {float(mr['median_depth']):.4f}" in out
        if mr["success"]:                          # scaled: the median depth of the map that stands is 1 to float accuracy
            n_maps += 1
            z = np.sort(made["points"][made["index"], 2])
            assert abs(float(z[(len(z) - 1) // 2]) - 1.0) <= 4 * 2.0 ** -23
            assert "kept, scaled to median depth 1" in out
        else:
            assert f"reset (reason {int(mr['reason'])})" in out
        ref = None
    assert n_init >= 1 and f"initialisations: {n_init}, initial maps kept: {n_maps}" in out
