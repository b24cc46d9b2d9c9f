"""Stereo rectification over the C ABI of liborbfe.so: cv::initUndistortRectifyMap once per camera and cv::remap(INTER_LINEAR) of
8-bit images, as Source/Examples/Stereo/stereo_euroc.cc:108-111, 159-160 of the reference does before TrackStereo.

The batch form runs on the device (rectify_kernels.hip); maps / coverage / rectify_image are host utilities (the same arithmetic,
byte for byte), not a fallback.  The arithmetic is this project's reading of OpenCV 4.5's scalar paths (include/orbfe.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import RectifyCamera

__all__ = ["RectifyCamera", "Rectifier", "rectify_camera", "rectifiers_from_settings"]


def rectify_camera(K, D, R, P, src_width: int, src_height: int, dst_width: int | None = None, dst_height: int | None = None) -> RectifyCamera:
    """orbfe_rectify_camera from K (3 x 3), D (k1 k2 p1 p2 k3), R (3 x 3), P (3 x 4); the destination defaults to the source size."""
    def flat(a, n, name):
        v = np.asarray(a, np.float64).ravel()
        if v.size != n:
            raise ValueError(f"{name} holds {v.size} values, expected {n}")
        return (C.c_double * n)(*v.tolist())
    return RectifyCamera(flat(K, 9, "K"), flat(D, 5, "D"), flat(R, 9, "R"), flat(P, 12, "P"), int(src_width), int(src_height),
                         int(src_width if dst_width is None else dst_width), int(src_height if dst_height is None else dst_height))


class Rectifier:
    """One camera's rectification maps.  device = -1: a host-only handle (maps, coverage, rectify_image; needs no GPU);
    device >= 0: the fixed-point map also lives on that device for rectify_batch."""

    def __init__(self, cam: RectifyCamera, device: int = -1):
        self._L = _lib.lib()
        self.cam, self.device = cam, int(device)
        self._h = C.c_void_p(None)
        _lib.check(self._L.orbfe_rectifier_create(C.byref(cam), self.device, C.byref(self._h)), "orbfe_rectifier_create")
        self.src_size = (cam.src_width, cam.src_height)
        self.dst_size = (cam.dst_width, cam.dst_height)

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def maps(self):
        """(map_x, map_y): float32 arrays of dst_height x dst_width."""
        w, h = self.dst_size
        mx, my = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
        _lib.check(self._L.orbfe_rectifier_maps(self._h, _lib.ptr(mx), _lib.ptr(my)), "orbfe_rectifier_maps")
        return mx, my

    def coverage(self):
        """(inner, edge, outside) destination pixel counts: all four taps inside the source / some / none."""
        c = [C.c_int32(0) for _ in range(3)]
        _lib.check(self._L.orbfe_rectifier_coverage(self._h, *(C.byref(x) for x in c)), "orbfe_rectifier_coverage")
        return tuple(x.value for x in c)

    def rectify_image(self, src: np.ndarray, out: np.ndarray | None = None) -> np.ndarray:
        """cv::remap of one host image (src_height x src_width uint8, rows contiguous, any row stride) on the CPU."""
        w, h = self.src_size
        if src.dtype != np.uint8 or src.ndim != 2 or src.shape != (h, w) or src.strides[1] != 1 or src.strides[0] < w:
            raise ValueError(f"source must be a {h} x {w} uint8 image with contiguous rows")
        dw, dh = self.dst_size
        if out is None:
            out = np.empty((dh, dw), np.uint8)
        if out.dtype != np.uint8 or out.shape != (dh, dw) or out.strides[1] != 1 or out.strides[0] < dw:
            raise ValueError(f"destination must be a {dh} x {dw} uint8 image with contiguous rows")
        _lib.check(self._L.orbfe_rectify_image(self._h, _lib.ptr(src), int(src.strides[0]), _lib.ptr(out), int(out.strides[0])),
                   "orbfe_rectify_image")
        return out

    def rectify_batch(self, src, dst, stream=None, n_images: int | None = None):
        """orbfe_rectify_batch_device on torch CUDA uint8 tensors: src (F, >= src_height, >= src_width) and dst
        (F, >= dst_height, >= dst_width) views; their row and image strides are the pitches and image strides, so padded
        blocks are passed as slices ([:, :h, :w]) of the padded tensors.  Asynchronous on `stream`."""
        for t, (w, h), name in ((src, self.src_size, "source"), (dst, self.dst_size, "destination")):
            if t.element_size() != 1 or t.dim() != 3 or t.shape[1] != h or t.shape[2] != w or (w > 1 and t.stride(2) != 1):
                raise ValueError(f"{name} must be an (F, {h}, {w}) uint8 tensor with contiguous rows")
        n = int(src.shape[0]) if n_images is None else int(n_images)
        if n > src.shape[0] or n > dst.shape[0]:
            raise ValueError("n_images exceeds the tensors")
        _lib.check(self._L.orbfe_rectify_batch_device(self._h, _lib.ptr(src), n, int(src.stride(1)), int(src.stride(0)), _lib.ptr(dst),
                                                      int(dst.stride(1)), int(dst.stride(0)), _lib.stream_handle(stream)),
                   "orbfe_rectify_batch_device")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.orbfe_rectifier_destroy(self._h)
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rectifiers_from_settings(path: str, device: int = -1):
    """(left, right) Rectifier objects from a stereo settings file (camera.read_stereo_rectification), as stereo_euroc.cc:108-111:
    each eye's map has that eye's LEFT. / RIGHT. width x height, which is also the size of its raw images."""
    from .camera import read_stereo_rectification
    s = read_stereo_rectification(path)
    out = []
    for eye in ("LEFT", "RIGHT"):
        c = s[eye]
        out.append(Rectifier(rectify_camera(c["K"], c["D"], c["R"], c["P"], c["width"], c["height"], c["width"], c["height"]), device))
    return tuple(out)
