"""CPU suite: the host side of the undistortion / image-bounds / RGB-D entry points (include/orbfe.h, csrc/frame_internal.h) against
the numpy second reading (tests/np_frames.py), bit for bit; a forward distortion model as a check independent of any transcription;
the settings reader; argument validation and the refusal without a device."""
import ctypes as C

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, camera
from tests import np_frames as nf


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _gpu_present(L):
    n = C.c_int(0)
    return L.orbfe_device_count(C.byref(n)) == 0 and n.value > 0


@pytest.mark.parametrize("name", sorted(nf.CAMERAS))
def test_undistort_points_equals_the_restatement(L, name):
    cal, (w, h) = nf.camera(name)
    pts = nf.dense_points(w, h)
    got = camera.undistort_points(cal, pts)
    exp, neg = nf.undistort(cal, pts, report=True)
    assert got.tobytes() == exp.tobytes()
    if name == "strong":
        assert neg.sum() > 100   # the icdist < 0 exit is taken
    else:
        assert not neg.any()
    assert not np.array_equal(got, pts)
    # in place
    buf = pts.copy()
    _lib.check(L.orbfe_undistort_points(C.byref(cal), _lib.ptr(buf), len(buf), _lib.ptr(buf)), "orbfe_undistort_points")
    assert buf.tobytes() == exp.tobytes()


@pytest.mark.parametrize("name", sorted(nf.CAMERAS) + ["tum3"])
def test_image_bounds_equal_the_restatement(name):
    cal, (w, h) = nf.camera(name)
    got = camera.image_bounds(cal, w, h)
    exp = nf.image_bounds(cal, w, h)
    assert np.array(got, np.float32).tobytes() == np.array(exp, np.float32).tobytes()
    if name == "tum1_rgbd":   # the issue's prototype: about (10.8, 626.1, 14.7, 473.3)
        np.testing.assert_allclose(got, (10.8, 626.05, 14.67, 473.31), atol=0.01)


def test_k1_zero_means_no_undistortion_whatever_the_rest():
    cal = camera.calibration(500, 500, 320, 240, 0.0, 0.3, 0.01, -0.02, 0.5, 40, 5000)
    pts = nf.dense_points(640, 480)
    assert camera.undistort_points(cal, pts).tobytes() == pts.tobytes()
    assert camera.image_bounds(cal, 640, 480) == (0.0, 640.0, 0.0, 480.0)
    assert camera.image_bounds(cal, 4095, 7) == (0.0, 4095.0, 0.0, 7.0)


@pytest.mark.parametrize("name", ["tum1_rgbd", "tum2_rgbd"])
def test_distorting_the_undistorted_point_gives_it_back(name):
    """independent of any transcription: a forward Brown-Conrady model in float64 maps the undistorted point back onto the
    keypoint, within 1e-3 px over the central 80 % of the image"""
    cal, (w, h) = nf.camera(name)
    xs = np.linspace(0.1 * w, 0.9 * w, 57); ys = np.linspace(0.1 * h, 0.9 * h, 43)
    pts = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2).astype(np.float32)
    back = nf.distort(cal, camera.undistort_points(cal, pts))
    assert np.abs(back - pts.astype(np.float64)).max() < 1e-3


def test_cross_check_against_opencv_when_present():
    cv2 = pytest.importorskip("cv2")
    for name in sorted(nf.CAMERAS):
        cal, (w, h) = nf.camera(name)
        K = np.array([[cal.fx, 0, cal.cx], [0, cal.fy, cal.cy], [0, 0, 1]], np.float32)
        D = np.array([cal.k1, cal.k2, cal.p1, cal.p2] + ([cal.k3] if cal.k3 != 0 else []), np.float32)
        pts = nf.dense_points(w, h).reshape(-1, 1, 2)
        exp = cv2.undistortPoints(pts, K, D, None, K).reshape(-1, 2)
        assert camera.undistort_points(cal, pts.reshape(-1, 2)).tobytes() == exp.astype(np.float32).tobytes(), name


def test_read_settings(tmp_path):
    p = tmp_path / "TUM1.yaml"
    p.write_text("%YAML:1.0\n\n# Camera calibration\nCamera.fx: 517.306408\nCamera.fy: 516.469215\nCamera.cx: 318.643040\n"
                 "Camera.cy: 255.313989\n\nCamera.k1: 0.262383\nCamera.k2: -0.953104\nCamera.p1: -0.005358\nCamera.p2: 0.002628\n"
                 "Camera.k3: 1.163314\n\nCamera.width: 640\nCamera.height: 480\nCamera.fps: 30.0\nCamera.bf: 40.0\nCamera.RGB: 1\n"
                 "ThDepth: 40.0\nDepthMapFactor: 5000.0\nORBextractor.nFeatures: 1000\nORBextractor.scaleFactor: 1.2\n"
                 "ORBextractor.nLevels: 8\nORBextractor.iniThFAST: 20\nORBextractor.minThFAST: 7\nViewer.PointSize:2\n")
    s = camera.read_settings(str(p))
    cal = s["calibration"]
    exp, _ = nf.camera("tum1_rgbd")
    assert bytes(cal) == bytes(exp)
    assert C.sizeof(cal) == 48 and np.float32(cal.depth_factor) == np.float32(1) / np.float32(5000)
    assert s["camera_rgb"] == 1 and (s["width"], s["height"]) == (640, 480)
    assert s["extractor"] == {"n_features": 1000, "scale_factor": float(np.float32(1.2)), "n_levels": 8, "ini_th_fast": 20, "min_th_fast": 7}
    # no k3 (the EuRoC / KITTI files), no DepthMapFactor (monocular): both read as 0, the factor as 1
    p.write_text("%YAML:1.0\nCamera.fx: 458.654\nCamera.fy: 457.296\nCamera.cx: 367.215\nCamera.cy: 248.375\nCamera.k1: -0.28340811\n"
                 "Camera.k2: 0.07395907\nCamera.p1: 0.00019359\nCamera.p2: 1.76187114e-05\nCamera.RGB: 1\n")
    s = camera.read_settings(str(p))
    assert bytes(s["calibration"]) == bytes(nf.camera("euroc_mono")[0]) and s["calibration"].k3 == 0 and s["calibration"].depth_factor == 1
    assert camera.depth_factor(5e-6) == 1 and camera.depth_factor(1.0) == 1 and camera.depth_factor(5208.0) == np.float32(1) / np.float32(5208)


def test_struct_layout_and_argument_validation(L):
    assert C.sizeof(_lib.Calibration) == 48
    cal, _ = nf.camera("tum1_rgbd")
    f = [C.c_float(7) for _ in range(4)]
    ok = lambda w, h: L.orbfe_image_bounds(C.byref(cal), w, h, *(C.byref(x) for x in f))
    assert ok(4095, 4095) == _lib.OK and ok(1, 1) == _lib.OK
    assert ok(4096, 480) == _lib.ERR_INVALID and ok(640, 4096) == _lib.ERR_INVALID and ok(0, 480) == _lib.ERR_INVALID
    assert L.orbfe_image_bounds(None, 640, 480, *(C.byref(x) for x in f)) == _lib.ERR_INVALID
    assert L.orbfe_image_bounds(C.byref(cal), 640, 480, None, C.byref(f[1]), C.byref(f[2]), C.byref(f[3])) == _lib.ERR_INVALID
    bad = _lib.Calibration.from_buffer_copy(bytes(cal)); bad.fx = 0
    assert L.orbfe_image_bounds(C.byref(bad), 640, 480, *(C.byref(x) for x in f)) == _lib.ERR_INVALID
    assert b"fx and fy" in L.orbfe_last_error()
    bad = _lib.Calibration.from_buffer_copy(bytes(cal)); bad.fy = 0
    xy = np.zeros((3, 2), np.float32)
    assert L.orbfe_undistort_points(C.byref(bad), _lib.ptr(xy), 3, _lib.ptr(xy)) == _lib.ERR_INVALID
    assert L.orbfe_undistort_points(C.byref(cal), None, 3, _lib.ptr(xy)) == _lib.ERR_INVALID
    assert L.orbfe_undistort_points(C.byref(cal), _lib.ptr(xy), -1, _lib.ptr(xy)) == _lib.ERR_INVALID
    assert L.orbfe_undistort_points(C.byref(cal), None, 0, None) == _lib.OK

    # the device entry point refuses bad arguments before it looks for a device; fake (never dereferenced) aligned pointers
    P = C.c_void_p(1 << 20)
    U16, F32 = _lib.DEPTH_U16, _lib.DEPTH_F32

    def dev(n_frames=2, kps=P, n=P, cap=1000, c=cal, fmt=U16, depth=P, w=640, h=480, pitch=1280, img=1280 * 480, kps_un=P, ur=P,
            dep=P, nd=P):
        return L.orbfe_undistort_frames_device(n_frames, kps, n, cap, None if c is None else C.byref(c), fmt, depth, w, h, pitch, img,
                                               kps_un, ur, dep, nd, None)
    for kw in ({"kps": None}, {"n": None}, {"kps_un": None}, {"c": None}, {"n_frames": -1}, {"cap": 0}, {"fmt": 3}, {"fmt": -1},
               {"depth": None}, {"ur": None}, {"dep": None}, {"nd": None}, {"w": 4096, "pitch": 8192, "img": 8192 * 480},
               {"h": 4096, "img": 1280 * 4096}, {"w": 0}, {"h": 0}, {"pitch": 1279}, {"img": 1280 * 479 + 1279},
               {"pitch": 1281, "img": 1281 * 480}, {"fmt": F32}, {"fmt": F32, "pitch": 2560, "img": 2560 * 480 - 2},
               {"depth": C.c_void_p((1 << 20) + 1)}, {"kps": C.c_void_p((1 << 20) + 2)}, {"c": bad}):
        assert dev(**kw) == _lib.ERR_INVALID, kw
    # the largest accepted map, the smallest accepted strides, DEPTH_NONE without depth buffers, n_frames = 0: valid -> no device here
    nodev = _lib.OK if _gpu_present(L) else _lib.ERR_NO_DEVICE
    if not _gpu_present(L):
        assert dev(w=4095, h=4095, pitch=8190, img=8190 * 4095) == nodev
        assert dev(fmt=F32, pitch=2560, img=2560 * 479 + 2560) == nodev
        assert dev(fmt=_lib.DEPTH_NONE, depth=None, ur=None, dep=None, nd=None, w=0, h=0, pitch=0, img=0) == nodev
        assert dev(n_frames=0) == nodev
        assert b"no CPU fallback" in L.orbfe_last_error()
