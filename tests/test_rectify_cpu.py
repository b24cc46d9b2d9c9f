"""CPU suite of stereo rectification (include/orbfe.h: orbfe_rectifier_*, orbfe_rectify_image; csrc/rectify_internal.h) on host-only
handles: the float maps, the pixel classes and the remapped bytes against the numpy second reading (tests/np_rectify.py), bit for
bit; two known answers that need no restatement; a float64 bilinear interpolation as a check independent of the fixed-point
arithmetic; the settings reader; every limit at its last accepted and first refused value."""
import ctypes as C

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, camera
from refactored_orb_slam2_amd.rectify import Rectifier, rectify_camera
from tests import np_rectify as nr

NAMES = sorted(nr.CAMERAS)


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def make(name, device=-1, **over):
    c = dict(nr.CAMERAS[name], **over)
    return Rectifier(rectify_camera(c["K"], c["D"], c["R"], c["P"], *c["src"], *c["dst"]), device)


def test_read_stereo_rectification(tmp_path):
    s = camera.read_stereo_rectification(nr.FIXTURE)
    mats = nr.read_fixture()
    assert len(mats) == 8
    for eye in ("LEFT", "RIGHT"):
        assert (s[eye]["width"], s[eye]["height"]) == (752, 480)
        for k, shape in (("K", (3, 3)), ("D", (1, 5)), ("R", (3, 3)), ("P", (3, 4))):
            assert s[eye][k].shape == shape and s[eye][k].dtype == np.float64
            assert s[eye][k].tobytes() == mats[f"{eye}.{k}"].tobytes()
    assert s["LEFT"]["K"][0][0] == 458.654 and s["LEFT"]["K"][1][2] == 248.375
    assert s["LEFT"]["D"][0][3] == 1.76187114e-05 and s["RIGHT"]["P"][0][3] == -47.90639384423901
    assert s["RIGHT"]["R"][0][0] == 0.9999633526194376 and s["RIGHT"]["R"][2][2] == 0.999945173484644
    # read_settings reads the same file's Camera.* / ORBextractor.* entries as before
    st = camera.read_settings(nr.FIXTURE)
    assert (st["width"], st["height"], st["extractor"]["n_features"]) == (752, 480, 1200)
    assert st["calibration"].mbf == np.float32(47.90639384423901)
    # data over several lines, `data: [` and `data:[`, comments
    text = open(nr.FIXTURE).read()
    multi = text.replace("0.0, 457.296, 248.375,", "0.0, 457.296,   # fy\n      248.375,")
    assert multi != text
    (tmp_path / "multi.yaml").write_text(multi)
    s2 = camera.read_stereo_rectification(str(tmp_path / "multi.yaml"))
    assert all(s2[e][k].tobytes() == s[e][k].tobytes() for e in ("LEFT", "RIGHT") for k in "KDRP")
    # where stereo_euroc.cc:98-104 stops: a matrix or a size is missing
    lines = text.splitlines(keepends=True)
    at = next(i for i, l in enumerate(lines) if l.startswith("RIGHT.R"))
    (tmp_path / "no_r.yaml").write_text("".join(lines[:at] + lines[at + 5:]))
    with pytest.raises(ValueError, match="RIGHT.R"):
        camera.read_stereo_rectification(str(tmp_path / "no_r.yaml"))
    (tmp_path / "no_h.yaml").write_text(text.replace("LEFT.height: 480", "LEFT.height: 0"))
    with pytest.raises(ValueError, match="LEFT.height"):
        camera.read_stereo_rectification(str(tmp_path / "no_h.yaml"))
    # more than five distortion coefficients cannot be expressed
    (tmp_path / "d8.yaml").write_text(text.replace("cols: 5\n   dt: d\n   data:[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]",
                                                   "cols: 8\n   dt: d\n   data:[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0, 0.1, 0.0, 0.0]"))
    with pytest.raises(ValueError, match="LEFT.D"):
        camera.read_stereo_rectification(str(tmp_path / "d8.yaml"))


@pytest.mark.parametrize("name", NAMES)
def test_maps_and_coverage_equal_the_restatement(L, name):
    c = nr.CAMERAS[name]
    mx, my = nr.camera_maps(name)
    with make(name) as r:
        gx, gy = r.maps()
        assert gx.shape == (c["dst"][1], c["dst"][0])
        assert gx.tobytes() == mx.tobytes() and gy.tobytes() == my.tobytes()
        inner, edge, outside = r.coverage()
    assert (inner, edge, outside) == nr.coverage(mx, my, *c["src"])
    assert inner + edge + outside == mx.size and inner > 0
    assert (edge > 0) == (name in nr.HAS_EDGE) and (outside > 0) == (name in nr.HAS_OUTSIDE)
    if name in nr.ALL_INNER:
        assert inner == mx.size
    if name == "euroc_right":
        assert (edge, outside) == (50, 0)


def test_euroc_maps_are_the_ones_the_issue_describes():
    mx, my = nr.camera_maps("euroc_left")
    np.testing.assert_allclose([mx.min(), mx.max(), my.min(), my.max()], [39.96, 696.80, 3.22, 466.46], atol=0.01)
    assert abs(float(nr.camera_maps("euroc_right")[1].max()) - 479.18) < 0.01


@pytest.mark.parametrize("name", NAMES)
def test_rectify_image_equals_the_restatement(L, name):
    c = nr.CAMERAS[name]
    mx, my = nr.camera_maps(name)
    w, h = c["src"]
    dw, dh = c["dst"]
    with make(name) as r:
        for k, kind in enumerate(("texture", "noise", "smooth")):
            src = nr.source(kind, w, h)
            exp = nr.remap(src, mx, my)
            assert r.rectify_image(src).tobytes() == exp.tobytes(), (name, kind)
            # strides larger than the widths; padding of the source holds other values, padding of the destination stays
            pad_s = np.full((h, w + 13 + k), 201, np.uint8)
            pad_s[:, :w] = src
            pad_d = np.full((dh, dw + 7 + k), 77, np.uint8)
            r.rectify_image(pad_s[:, :w], pad_d[:, :dw])
            assert pad_d[:, :dw].tobytes() == exp.tobytes(), (name, kind, "strided")
            assert (pad_d[:, dw:] == 77).all()
        if name in nr.HAS_OUTSIDE:
            assert (r.rectify_image(np.full((h, w), 255, np.uint8)) == 0).any()


def test_known_answers(L):
    w, h = nr.SRC_W, nr.SRC_H
    for kind in ("texture", "noise", "smooth"):
        src = nr.source(kind, w, h, seed=1)
        with make("identity") as r:
            assert np.array_equal(r.rectify_image(src), src)
        s = src.astype(np.int32)
        exp = np.empty_like(s)
        exp[:, :w - 1] = (s[:, :w - 1] + s[:, 1:] + 1) >> 1
        exp[:, w - 1] = (s[:, w - 1] + 1) >> 1
        with make("half_pixel") as r:
            assert np.array_equal(r.rectify_image(src), exp.astype(np.uint8))


@pytest.mark.parametrize("name", ["euroc_left", "euroc_right"])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_independent_float64_bilinear_check(L, name, kind):
    """|out - B| <= g / 32 + 0.52 on every inner pixel: B the float64 bilinear value, g the largest step between adjacent source
    pixels around the pixel's cell.  Each coordinate is rounded to 1/32 (at most 1/64 off per axis, slope at most g per axis);
    rounding may move the cell by one (hence the 3 x 3 block of cells); 0.5 is the final rounding, 0.02 the integer weights."""
    c = nr.CAMERAS[name]
    mx, my = nr.camera_maps(name)
    src = nr.source(kind, *c["src"])
    with make(name) as r:
        out = r.rectify_image(src).astype(np.float64)
    _, _, _, _, _, inner, _, _ = nr.fixed_point(mx, my, *c["src"])
    assert inner.mean() >= 0.9998 and (~inner).sum() <= 50
    B, x0, y0 = nr.bilinear64(src, mx, my)
    bound = nr.local_gradient(src, x0, y0) / 32.0 + 0.52
    ratio = (np.abs(out - B) / bound)[inner]
    print(f"{name} {kind}: largest |out - B| / bound = {ratio.max():.4f}, largest |out - B| = {np.abs(out - B)[inner].max():.4f}")
    assert (ratio <= 1.0).all()


def _cam(sw=8, sh=6, dw=8, dh=6, **over):
    c = dict(nr.CAMERAS["identity"], **over)
    return rectify_camera(c["K"], c["D"], c["R"], c["P"], sw, sh, dw, dh)


def _create(L, cam, device=-1):
    h = C.c_void_p(None)
    rc = L.orbfe_rectifier_create(C.byref(cam), device, C.byref(h))
    return rc, h


def test_limits_at_their_boundaries(L):
    assert C.sizeof(_lib.RectifyCamera) == 296
    src = np.arange(48, dtype=np.uint8).reshape(6, 8)

    def still_works():
        with Rectifier(_cam()) as r:
            K = nr.CAMERAS["identity"]["K"]
            assert r.coverage()[0] > 0 and r.rectify_image(src).shape == (6, 8)
            assert K[0, 2] > 8   # the identity camera's centre is far right of this tiny image; the map is still the identity
            assert np.array_equal(r.rectify_image(src), src)

    # sizes: 1 .. 4095 per side, each of the four on its own
    for field in ("sw", "sh", "dw", "dh"):
        for v, ok in ((1, True), (4095, True), (0, False), (4096, False), (-1, False)):
            rc, h = _create(L, _cam(**{field: v}))
            if ok:
                assert rc == _lib.OK and h.value, (field, v)
                assert L.orbfe_rectifier_destroy(h) == _lib.OK
            else:
                assert rc == _lib.ERR_INVALID and not h.value, (field, v)
                assert b"4095" in L.orbfe_last_error()
            still_works()
    # the largest map on the host: 4095 x 4095 from a 4095 x 4095 source, identity -> the source itself
    big = nr.source("noise", 4095, 4095)
    with Rectifier(_cam(4095, 4095, 4095, 4095)) as r:
        assert r.coverage() == (4094 * 4094, 2 * 4095 - 1, 0)
        assert np.array_equal(r.rectify_image(big), big)
    # a skewed K, a singular P x R
    K = np.array(nr.CAMERAS["identity"]["K"], copy=True)
    K[0, 1] = 1e-9
    rc, h = _create(L, _cam(K=K))
    assert rc == _lib.ERR_INVALID and b"skew" in L.orbfe_last_error()
    P = np.array(nr.CAMERAS["identity"]["P"], copy=True)
    P[1, :] = 2 * P[0, :]
    rc, h = _create(L, _cam(P=P))
    assert rc == _lib.ERR_INVALID and b"singular" in L.orbfe_last_error()
    still_works()
    # null arguments, a device index below -1
    assert L.orbfe_rectifier_create(None, -1, C.byref(C.c_void_p())) == _lib.ERR_INVALID
    assert _create(L, _cam(), device=-2)[0] == _lib.ERR_INVALID and b"device" in L.orbfe_last_error()
    # host image: each stride at least its width
    with Rectifier(_cam()) as r:
        dst = np.zeros((6, 8), np.uint8)
        a = (r.handle, _lib.ptr(src), 8, _lib.ptr(dst), 8)
        assert L.orbfe_rectify_image(*a) == _lib.OK
        assert L.orbfe_rectify_image(r.handle, _lib.ptr(src), 7, _lib.ptr(dst), 8) == _lib.ERR_INVALID and b"stride" in L.orbfe_last_error()
        assert L.orbfe_rectify_image(r.handle, _lib.ptr(src), 8, _lib.ptr(dst), 7) == _lib.ERR_INVALID and b"stride" in L.orbfe_last_error()
        assert L.orbfe_rectify_image(r.handle, None, 8, _lib.ptr(dst), 8) == _lib.ERR_INVALID
        assert L.orbfe_rectify_image(*a) == _lib.OK and np.array_equal(dst, src)
        # a host-only handle has no device side: the batch entry point refuses it, there is no CPU fallback
        rc = L.orbfe_rectify_batch_device(r.handle, _lib.ptr(src), 1, 8, 48, _lib.ptr(dst), 8, 48, None)
        assert rc == _lib.ERR_NO_DEVICE and b"host-only" in L.orbfe_last_error()
        assert L.orbfe_rectify_image(*a) == _lib.OK
    still_works()


def test_single_row_and_single_column_sources(L):
    """A 1-pixel-wide or 1-pixel-high source has no inner pixel; every tap check is exercised (nothing outside the source is read:
    the source array ends with the image)."""
    for (sw, sh, dw, dh) in ((1, 9, 5, 9), (9, 1, 9, 4), (1, 1, 3, 3)):
        c = nr.CAMERAS["half_pixel"]
        src = nr.source("noise", sw, sh)
        mx, my = nr.init_maps(c["K"], c["D"], c["R"], c["P"], dw, dh)
        with Rectifier(rectify_camera(c["K"], c["D"], c["R"], c["P"], sw, sh, dw, dh)) as r:
            assert r.coverage() == nr.coverage(mx, my, sw, sh) and r.coverage()[0] == 0
            assert r.rectify_image(src).tobytes() == nr.remap(src, mx, my).tobytes()
