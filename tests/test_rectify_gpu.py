"""GPU suite of stereo rectification: orbfe_rectify_batch_device (csrc/rectify_kernels.hip) against the numpy second reading
(tests/np_rectify.py) byte for byte on pitched, padded batches; batch against image-by-image calls; the largest sizes; the limits of
the device entry point at their boundaries; the rectification stage of the pipeline handle against the same handle fed rectified
images; examples/stereo_euroc.py on a synthetic EuRoC layout against the oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from refactored_orb_slam2_amd import _lib, synth
from refactored_orb_slam2_amd.rectify import Rectifier, rectifiers_from_settings, rectify_camera
from tests import np_rectify as nr
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(nr.CAMERAS)
MARK = 0xA5


def make(name, device=0):
    c = nr.CAMERAS[name]
    return Rectifier(rectify_camera(c["K"], c["D"], c["R"], c["P"], *c["src"], *c["dst"]), device)


def _sources(n, w, h):
    kinds = ("texture", "noise", "smooth")
    return [nr.source(kinds[i % 3], w, h, seed=i) for i in range(n)]


def _run_padded(r, imgs, sw, sh, dw, dh, spitch, sstride, dpitch, dstride, stream=None):
    """The images in a source block that ends with the last image's last byte, through the C entry point into a destination block
    filled with MARK; returns the whole destination block as (n, dstride) host bytes."""
    import torch
    n = len(imgs)
    sbytes = (n - 1) * sstride + (sh - 1) * spitch + sw
    host = np.full(sbytes, 0x3C, np.uint8)
    for i, im in enumerate(imgs):
        for y in range(sh):
            o = i * sstride + y * spitch
            host[o:o + sw] = im[y]
    d_src = torch.from_numpy(host).cuda()
    d_dst = torch.full((n * dstride,), MARK, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # the fill ran on torch's stream, the kernel runs on another
    s = torch.cuda.Stream() if stream is None else stream
    _lib.check(_lib.lib().orbfe_rectify_batch_device(r.handle, _lib.ptr(d_src), n, spitch, sstride, _lib.ptr(d_dst), dpitch, dstride,
                                                     _lib.stream_handle(s)), "orbfe_rectify_batch_device")
    s.synchronize()
    return d_dst.cpu().numpy().reshape(n, dstride)


def _check_block(block, exp, dw, dh, dpitch):
    """block: (n, dstride) bytes; exp: list of (dh, dw) images.  The images equal exp, everything else still holds MARK."""
    n, dstride = block.shape
    rows = block[:, :dh * dpitch].reshape(n, dh, dpitch)
    for i, e in enumerate(exp):
        assert rows[i, :, :dw].tobytes() == e.tobytes(), f"image {i}"
    assert (rows[:, :-1, dw:] == MARK).all(), "row padding was written"
    tail = block[:, (dh - 1) * dpitch + dw:]
    assert (tail == MARK).all(), "bytes behind an image were written"


@pytest.mark.parametrize("name", NAMES)
def test_batch_equals_the_restatement_on_padded_blocks(name):
    c = nr.CAMERAS[name]
    (sw, sh), (dw, dh) = c["src"], c["dst"]
    mx, my = nr.camera_maps(name)
    imgs = _sources(5, sw, sh)
    exp = [nr.remap(im, mx, my) for im in imgs]
    with make(name) as r:
        assert r.coverage() == nr.coverage(mx, my, sw, sh)
        k = NAMES.index(name)
        # pitches / strides that are multiples of 4 (dword stores) and ones that are not (byte stores), by camera
        for spitch, dpitch, extra in ((sw + 16 + 4 * k, dw + 32, 128), (sw + 3 + k, dw + 5 + 2 * (k % 3), 77)):
            sstride, dstride = spitch * sh + extra, dpitch * dh + extra + 4
            block = _run_padded(r, imgs, sw, sh, dw, dh, spitch, sstride, dpitch, dstride)
            _check_block(block, exp, dw, dh, dpitch)


def test_batch_equals_single_calls_and_repeats():
    import torch
    name = "euroc_right"
    c = nr.CAMERAS[name]
    (sw, sh), (dw, dh) = c["src"], c["dst"]
    mx, my = nr.camera_maps(name)
    base = _sources(7, sw, sh)
    s = torch.cuda.Stream()
    with make(name) as r, torch.cuda.stream(s):   # torch's own kernels (fills, gathers, comparisons) on the same stream
        src = torch.from_numpy(np.stack(base)).cuda()
        one = torch.zeros((7, dh, dw), dtype=torch.uint8, device="cuda")
        for i in range(7):
            r.rectify_batch(src[i:i + 1], one[i:i + 1], s)
        allb = torch.zeros_like(one)
        r.rectify_batch(src, allb, s)
        again = torch.zeros_like(one)
        r.rectify_batch(src, again, s)
        s.synchronize()
        assert torch.equal(one, allb) and torch.equal(allb, again)
        assert one[3].cpu().numpy().tobytes() == nr.remap(base[3], mx, my).tobytes()
        # n_images = 0: nothing is launched, nothing is touched -- not even the pointers
        marked = torch.full((2, dh, dw), MARK, dtype=torch.uint8, device="cuda")
        r.rectify_batch(src, marked, s, n_images=0)
        assert _lib.lib().orbfe_rectify_batch_device(r.handle, None, 0, sw, sw * sh, None, dw, dw * dh, _lib.stream_handle(s)) == _lib.OK
        s.synchronize()
        assert bool((marked == MARK).all())
        # a batch of 256 (each workgroup walks many images with its map entries in registers) and a batch of 1
        idx = np.arange(256) % 7
        big = src[torch.from_numpy(idx).cuda()].contiguous()
        out = torch.zeros((256, dh, dw), dtype=torch.uint8, device="cuda")
        r.rectify_batch(big, out, s)
        s.synchronize()
        assert torch.equal(out, allb[torch.from_numpy(idx).cuda()])
        single = torch.zeros((1, dh, dw), dtype=torch.uint8, device="cuda")
        r.rectify_batch(src[5:6], single, s)
        s.synchronize()
        assert torch.equal(single[0], allb[5])


def _big_camera(sw, sh, dw, dh):
    f = 0.8 * max(sw, sh)
    K = np.array([[f, 0, sw / 2], [0, f, sh / 2], [0, 0, 1]], np.float64)
    P = nr._p(0.95 * f, 0.95 * f, dw / 2 - 0.4, dh / 2 + 0.3)
    return dict(K=K, D=np.array([-0.05, 0.01, 0.0003, -0.0002, 0.002]), R=nr._rz(0.3), P=P)


@pytest.mark.parametrize("size", [(4095, 4095), (4095, 1), (1, 4095)])
def test_largest_sizes(size):
    """4095 x 4095, 4095 x 1 and 1 x 4095 (width x height) sources and destinations, each once, against the restatement."""
    w, h = size
    c = _big_camera(w, h, w, h)
    mx, my = nr.init_maps(c["K"], c["D"], c["R"], c["P"], w, h)
    src = nr.source("noise", w, h, seed=4)
    exp = nr.remap(src, mx, my)
    with Rectifier(rectify_camera(c["K"], c["D"], c["R"], c["P"], w, h, w, h), 0) as r:
        cov = r.coverage()
        assert cov == nr.coverage(mx, my, w, h)
        if min(w, h) > 1:
            assert min(cov) > 0   # inner, edge and outside pixels all occur
        block = _run_padded(r, [src], w, h, w, h, w + 1, (w + 1) * h + 9, w + 4, (w + 4) * h + 8)
        _check_block(block, [exp], w, h, w + 4)


def test_device_limits_at_their_boundaries():
    import torch
    L = _lib.lib()
    c = nr.CAMERAS["identity"]
    sw, sh, dw, dh = 40, 12, 36, 10
    src_img = nr.source("noise", sw, sh)
    mx, my = nr.init_maps(c["K"], c["D"], c["R"], c["P"], dw, dh)
    exp = nr.remap(src_img, mx, my)
    s = torch.cuda.Stream()
    sh_ = _lib.stream_handle(s)
    with Rectifier(rectify_camera(c["K"], c["D"], c["R"], c["P"], sw, sh, dw, dh), 0) as r, torch.cuda.stream(s):
        n = 3
        d_src = torch.from_numpy(np.stack([src_img] * n)).cuda()
        d_dst = torch.zeros((n, dh, dw), dtype=torch.uint8, device="cuda")

        def call(spitch=sw, sstride=sw * sh, dpitch=dw, dstride=dw * dh, src=None, dst=None, count=n):
            return L.orbfe_rectify_batch_device(r.handle, _lib.ptr(d_src) if src is None else src, count, spitch, sstride,
                                                _lib.ptr(d_dst) if dst is None else dst, dpitch, dstride, sh_)

        def still_works():
            d_dst.zero_()
            assert call() == _lib.OK
            s.synchronize()
            assert all(d_dst[i].cpu().numpy().tobytes() == exp.tobytes() for i in range(n))

        still_works()
        # pitches: the width is the last accepted value
        assert call(spitch=sw - 1) == _lib.ERR_INVALID and b"pitch" in L.orbfe_last_error()
        assert call(dpitch=dw - 1) == _lib.ERR_INVALID and b"pitch" in L.orbfe_last_error()
        still_works()
        # image strides: (height - 1) * pitch + width is the last accepted value (one image with a pitch above the width, inside
        # the three-image tensors)
        sp, dp = sw + 2, dw + 2
        assert call(spitch=sp, sstride=(sh - 1) * sp + sw, count=1) == _lib.OK
        assert call(spitch=sp, sstride=(sh - 1) * sp + sw - 1, count=1) == _lib.ERR_INVALID and b"stride" in L.orbfe_last_error()
        assert call(dpitch=dp, dstride=(dh - 1) * dp + dw, count=1) == _lib.OK
        assert call(dpitch=dp, dstride=(dh - 1) * dp + dw - 1, count=1) == _lib.ERR_INVALID and b"stride" in L.orbfe_last_error()
        s.synchronize()
        still_works()
        # overlap: a destination that begins on the source's last byte is refused, one that begins right behind it is accepted
        blk = torch.zeros(n * sw * sh + n * dw * dh, dtype=torch.uint8, device="cuda")
        blk[:n * sw * sh].copy_(d_src.reshape(-1))
        base = blk.data_ptr()
        end_src = n * sw * sh
        assert call(src=C.c_void_p(base), dst=C.c_void_p(base + end_src - 1)) == _lib.ERR_INVALID and b"overlap" in L.orbfe_last_error()
        assert call(src=C.c_void_p(base), dst=C.c_void_p(base)) == _lib.ERR_INVALID
        assert call(src=C.c_void_p(base), dst=C.c_void_p(base + end_src)) == _lib.OK
        s.synchronize()
        got = blk[end_src:].cpu().numpy().reshape(n, dh, dw)
        assert all(got[i].tobytes() == exp.tobytes() for i in range(n))
        # ... and the other way round: the source right behind the destination
        blk2 = torch.zeros(n * dw * dh + n * sw * sh, dtype=torch.uint8, device="cuda")
        blk2[n * dw * dh:].copy_(d_src.reshape(-1))
        b2 = blk2.data_ptr()
        assert call(src=C.c_void_p(b2 + n * dw * dh), dst=C.c_void_p(b2)) == _lib.OK
        assert call(src=C.c_void_p(b2 + n * dw * dh - 1), dst=C.c_void_p(b2)) == _lib.ERR_INVALID and b"overlap" in L.orbfe_last_error()
        s.synchronize()
        # negative counts, missing pointers
        assert call(count=-1) == _lib.ERR_INVALID
        assert call(src=C.c_void_p(None)) == _lib.ERR_INVALID and b"required" in L.orbfe_last_error()
        still_works()
    # a host-only handle on a machine WITH a device is still refused: there is no CPU fallback
    with Rectifier(rectify_camera(c["K"], c["D"], c["R"], c["P"], sw, sh, dw, dh), -1) as r:
        rc = L.orbfe_rectify_batch_device(r.handle, _lib.ptr(d_src), 1, sw, sw * sh, _lib.ptr(d_dst), dw, dw * dh, sh_)
        assert rc == _lib.ERR_NO_DEVICE and b"host-only" in L.orbfe_last_error()
    # a device that does not exist
    h = C.c_void_p(None)
    cam = rectify_camera(c["K"], c["D"], c["R"], c["P"], sw, sh, dw, dh)
    assert L.orbfe_rectifier_create(C.byref(cam), 4096, C.byref(h)) == _lib.ERR_INVALID and not h.value


OUT_KEYS = ("n_left", "n_right", "n_stereo", "n_tracked", "kps_left", "desc_left", "u_right", "depth", "assigned")


def _snapshot(out, n):
    snap = {}
    for k in OUT_KEYS:
        a = np.asarray(out[k])
        if a.ndim == 1:
            snap[k] = a[:n].copy()
        else:
            snap[k] = [a[j, :int(out["n_left"][j])].copy() for j in range(n)]
    return snap


def _same(a, b, what):
    for k in OUT_KEYS:
        if isinstance(a[k], list):
            for j, (x, y) in enumerate(zip(a[k], b[k])):
                assert x.tobytes() == y.tobytes(), (what, k, j)
        else:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_pipeline_with_rectifiers_equals_the_pipeline_on_rectified_images():
    from refactored_orb_slam2_amd import camera
    from refactored_orb_slam2_amd.pipeline import StereoPipeline
    W, H, NF, F, N = 752, 480, 1200, 3, 6
    st = camera.read_settings(nr.FIXTURE)
    cal = st["calibration"]
    raw = synth.sequence(W, H, N, seq=37, stereo=True)
    ml, mr = nr.camera_maps("euroc_left"), nr.camera_maps("euroc_right")
    rect = [(nr.remap(l, *ml), nr.remap(r, *mr)) for l, r in raw]
    assert any(not np.array_equal(rect[i][0], raw[i][0]) for i in range(N))
    args = (W, H, F, cal.fx, cal.fy, cal.cx, cal.cy, cal.mbf, 7.0)
    rl, rr = rectifiers_from_settings(nr.FIXTURE, device=0)

    def run(p, pairs, resident=False):
        snaps = []
        for k in range(2):
            idx = list(range(3 * k, 3 * k + 3))
            if not resident:
                for j, i in enumerate(idx):
                    p.left(k)[j, :, :W] = pairs[i][0]
                    p.right(k)[j, :, :W] = pairs[i][1]
                p.submit(k, 3, has_predecessor=k > 0)
            else:
                p.submit_resident(k, 3, has_predecessor=k > 0)
            p.wait(k)
            snaps.append(_snapshot(p.output(k), 3))
        return snaps

    with StereoPipeline(*args, n_features=NF, slots=2) as ref:
        exp = run(ref, rect)
    assert min(int(s["n_left"].min()) for s in exp) > 500 and int(exp[1]["n_tracked"].sum()) > 100 and int(exp[0]["n_stereo"].sum()) > 100
    with StereoPipeline(*args, n_features=NF, slots=2) as p:
        # rectifiers of another size, a host-only rectifier
        c = nr.CAMERAS["crop_up"]
        with Rectifier(rectify_camera(c["K"], c["D"], c["R"], c["P"], *c["src"], *c["dst"]), 0) as other, make("euroc_left", -1) as host:
            with pytest.raises(_lib.OrbfeError, match="752 x 480"):
                p.set_rectifiers(rl, other)
            with pytest.raises(_lib.OrbfeError, match="device"):
                p.set_rectifiers(host, rr)
        p.set_rectifiers(rl, rr)
        got = run(p, raw)
        for k in range(2):
            _same(got[k], exp[k], f"submit, chunk {k}")
        # the raw images stay in the slots' device blocks: resident submits rectify them again; host frames overwritten to prove
        # that nothing is uploaded
        p.left(0)[1, :, :W] = 0
        p.right(1)[2, :, :W] = 255
        again = run(p, raw, resident=True)
        for k in range(2):
            _same(again[k], exp[k], f"submit_resident, chunk {k}")
        with pytest.raises(_lib.OrbfeError, match="before the first submit"):
            p.set_rectifiers(rl, rr)
    # after a submit the stage cannot be added any more
    with StereoPipeline(*args, n_features=NF, slots=1) as p:
        p.submit(0, 1, has_predecessor=False)
        p.wait(0)
        with pytest.raises(_lib.OrbfeError, match="before the first submit"):
            p.set_rectifiers(rl, rr)
    # raw images through a handle without rectifiers give other results: the stage is not a no-op on this data
    with StereoPipeline(*args, n_features=NF, slots=2) as p:
        unrect = run(p, raw)
    assert any(unrect[k]["kps_left"][j].tobytes() != exp[k]["kps_left"][j].tobytes() for k in range(2) for j in range(3))
    rl.close(); rr.close()


def test_stereo_euroc_driver_on_a_synthetic_euroc_layout(tmp_path):
    """examples/stereo_euroc.py on a EuRoC layout written by tools/make_euroc_layout.py (raw PNG pairs named by their stamps, a stamp
    file) with the reference's EuRoC settings file: per-frame mode and batches of 4 and 2 over 5 frames (neither divides the frame
    count).  The dumped rectified pairs == the restatement; every frame's dump == the oracle run on the restatement's images."""
    from refactored_orb_slam2_amd import camera
    from refactored_orb_slam2_amd._lib import TRACK_POSE_DTYPE, UNPROJECT_CAM_DTYPE
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_euroc_layout
    W, H, N = 752, 480, 5
    seq = tmp_path / "mav0"
    raw = synth.sequence(W, H, N, seq=41, stereo=True)
    stamps = make_euroc_layout.write_layout(str(seq), raw)
    assert sorted(os.listdir(seq / "cam0" / "data")) == [f"{s}.png" for s in stamps]
    ml, mr = nr.camera_maps("euroc_left"), nr.camera_maps("euroc_right")
    rect = [(nr.remap(l, *ml), nr.remap(r, *mr)) for l, r in raw]
    st = camera.read_settings(nr.FIXTURE)
    cal, ep = st["calibration"], st["extractor"]
    NF = ep["n_features"]
    assert NF == 1200
    oL = ol.OracleExtractor(NF, ep["scale_factor"], ep["n_levels"], ep["ini_th_fast"], ep["min_th_fast"])
    oR = ol.OracleExtractor(NF, ep["scale_factor"], ep["n_levels"], ep["ini_th_fast"], ep["min_th_fast"])
    sf, isf = oL.scale_factors, oL.inv_scale_factors
    fx, fy, cx, cy, bf = cal.fx, cal.fy, cal.cx, cal.cy, cal.mbf
    cam = np.zeros(1, UNPROJECT_CAM_DTYPE); pose = np.zeros(1, TRACK_POSE_DTYPE)
    eye = np.eye(3, dtype=np.float32).reshape(9)
    cam["Rwc"] = eye; cam["cx"] = cx; cam["cy"] = cy; cam["invfx"] = np.float32(1) / np.float32(fx); cam["invfy"] = np.float32(1) / np.float32(fy)
    pose["Rcw"] = eye; pose["fx"] = fx; pose["fy"] = fy; pose["cx"] = cx; pose["cy"] = cy; pose["mbf"] = bf
    pose["max_x"] = W; pose["max_y"] = H; pose["th"] = 7.0; pose["scale_factors"][0, :8] = sf
    exp, prev = [], None
    for (Li, Ri) in rect:
        kL, dL = oL(Li); kR, dR = oR(Ri)
        _, ur, depth = ol.compute_stereo_matches(kL, dL, kR, dR, [oL.level_pixels(l) for l in range(8)], [oR.level_pixels(l) for l in range(8)],
                                                 sf, isf, bf, bf / fx)
        nm, assigned = 0, np.full(len(kL), -1, np.int32)
        if prev is not None:
            nm, assigned, _ = ol.OracleFrame(kL, dL, sf, 0, W, 0, H, ur).search_by_projection_frame(ol.track_queries(pose, prev), True)
        exp.append((kL, dL, ur, depth, nm, assigned))
        prev = ol.unproject_stereo(cam, kL, dL, depth)
    drv = os.path.join(ROOT, "examples", "stereo_euroc.py")
    for extra in ([], ["--batch", "4"], ["--batch", "2"]):
        dump = str(tmp_path / "dump.npz")
        r = subprocess.run([sys.executable, drv, str(seq / "cam0" / "data"), str(seq / "cam1" / "data"), str(seq / "stamps.txt"), nr.FIXTURE,
                            "--dump", dump] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "median tracking time" in r.stdout and "Images in the sequence: 5" in r.stdout
        g = np.load(dump)
        for i, (kL, dL, ur, depth, nm, assigned) in enumerate(exp):
            assert g[f"rect_left_{i}"].tobytes() == rect[i][0].tobytes() and g[f"rect_right_{i}"].tobytes() == rect[i][1].tobytes(), (i, extra)
            assert float(g[f"time_{i}"]) == stamps[i] / 1e9
            np.testing.assert_array_equal(g[f"kp_{i}"], kL, err_msg=f"keypoints of frame {i} ({extra})")
            np.testing.assert_array_equal(g[f"desc_{i}"], dL)
            np.testing.assert_array_equal(g[f"ur_{i}"], ur); np.testing.assert_array_equal(g[f"depth_{i}"], depth)
            assert int(g[f"ntrack_{i}"]) == nm, (i, extra)
            np.testing.assert_array_equal(g[f"assigned_{i}"], assigned)
    assert min(len(e[0]) for e in exp) > 500 and sum(int((e[2] >= 0).sum()) for e in exp) > 100
    # --max-frames, and a settings file without the rectification entries stops the driver as the reference's does
    r = subprocess.run([sys.executable, drv, str(seq / "cam0" / "data"), str(seq / "cam1" / "data"), str(seq / "stamps.txt"), nr.FIXTURE,
                        "--max-frames", "2", "--batch", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Images in the sequence: 2" in r.stdout
    bad = tmp_path / "bad.yaml"
    bad.write_text(open(nr.FIXTURE).read().replace("RIGHT.width: 752", "RIGHT.width: 0"))
    r = subprocess.run([sys.executable, drv, str(seq / "cam0" / "data"), str(seq / "cam1" / "data"), str(seq / "stamps.txt"), str(bad)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Calibration parameters to rectify stereo are missing" in r.stderr
