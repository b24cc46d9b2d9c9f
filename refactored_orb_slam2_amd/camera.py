"""The camera side of Frame::Frame over the C ABI of liborbfe.so: lens undistortion of the keypoints (UndistortKeyPoints), the
image bounds (ComputeImageBounds) and the RGB-D depth of every keypoint (ComputeStereoFromRGBD), plus a reader of the reference's
settings files.

L/src/Frame.cc:419-476, 648-666 and L/src/Tracking.cc:43-147, 193-211 (L/ = Source/Libraries/ORB_SLAM2/).  The batch form runs on
the device (frame_kernels.hip); image_bounds / undistort_points are host utilities for calibration time (the same arithmetic, bit
for bit), not a fallback.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import _lib
from ._lib import DEPTH_F32, DEPTH_NONE, DEPTH_U16, Calibration

__all__ = ["Calibration", "DEPTH_NONE", "DEPTH_U16", "DEPTH_F32", "calibration", "depth_factor", "image_bounds", "undistort_points",
           "undistort_frames_batch", "read_settings", "read_stereo_rectification"]


def depth_factor(depth_map_factor) -> np.float32:
    """mDepthMapFactor of Tracking (L/src/Tracking.cc:141-147): 1.0f / DepthMapFactor, or 1 when |DepthMapFactor| < 1e-5 (float)."""
    f = np.float32(depth_map_factor)
    if float(np.abs(f)) < 1e-5:
        return np.float32(1)
    return np.float32(np.float32(1) / f)


def calibration(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, bf=0.0, depth_map_factor=0.0) -> Calibration:
    """orbfe_calibration from the values of a settings file (depth_map_factor = DepthMapFactor, 0 / absent: no scaling)."""
    return Calibration(*(float(np.float32(v)) for v in (fx, fy, cx, cy, k1, k2, p1, p2, k3, bf)),
                       float(depth_factor(depth_map_factor)), 0)


def image_bounds(cal: Calibration, width: int, height: int):
    """ComputeImageBounds (Frame.cc:447-476): (mnMinX, mnMaxX, mnMinY, mnMaxY) as Python floats holding float32 values."""
    b = [C.c_float(0) for _ in range(4)]
    _lib.check(_lib.lib().orbfe_image_bounds(C.byref(cal), int(width), int(height), *(C.byref(x) for x in b)), "orbfe_image_bounds")
    return tuple(x.value for x in b)


def undistort_points(cal: Calibration, xy) -> np.ndarray:
    """cv::undistortPoints(pts, pts, mK, mDistCoef, cv::Mat(), mK) of (n, 2) float points; returns (n, 2) float32."""
    pts = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.empty_like(pts)
    _lib.check(_lib.lib().orbfe_undistort_points(C.byref(cal), _lib.ptr(pts), len(pts), _lib.ptr(out)), "orbfe_undistort_points")
    return out


def undistort_frames_batch(kps, n, cal: Calibration, depth_format: int, depth, kps_un, u_right=None, depth_out=None, n_depth=None,
                           stream=None, width: int | None = None):
    """orbfe_undistort_frames_device on torch CUDA tensors: kps / kps_un (F,cap,28) u8 (kps_un may be kps), n (F) i32; with
    DEPTH_U16 / DEPTH_F32: depth (F, H, W') of 2- / 4-byte samples (its row and image strides are the map's pitch and stride; width
    defaults to W'), u_right / depth_out (F,cap) f32 and n_depth (F) i32.  DEPTH_NONE: depth None, the three outputs optional."""
    F, cap = kps.shape[0], kps.shape[1]
    w = h = pitch = image_bytes = 0
    if depth is not None:
        es = depth.element_size()
        if es != (2 if depth_format == DEPTH_U16 else 4):
            raise ValueError(f"depth tensor of {es}-byte samples does not fit depth format {depth_format}")
        h, w = int(depth.shape[1]), int(depth.shape[2] if width is None else width)
        pitch, image_bytes = int(depth.stride(1)) * es, int(depth.stride(0)) * es
    _lib.check(_lib.lib().orbfe_undistort_frames_device(F, _lib.ptr(kps), _lib.ptr(n), cap, C.byref(cal), int(depth_format),
                                                        _lib.ptr(depth), w, h, pitch, image_bytes, _lib.ptr(kps_un), _lib.ptr(u_right),
                                                        _lib.ptr(depth_out), _lib.ptr(n_depth), _lib.stream_handle(stream)),
               "orbfe_undistort_frames_device")


_ENTRY = re.compile(r"^\s*([A-Za-z_][A-Za-z0-9_.]*)\s*:\s*(.*?)\s*$")


def read_settings(path: str) -> dict:
    """The reference's settings file (%YAML:1.0, one `Key: value` per line; e.g. Source/Examples/RGB-D/TUM1.yaml) without OpenCV.
    Reads what Tracking's constructor does (L/src/Tracking.cc:43-147): Camera.fx .. cy, k1, k2, p1, p2, k3 (optional, 0), bf,
    RGB, width / height (when present), DepthMapFactor (0 when absent: no scaling), ThDepth and the ORBextractor.* parameters.
    A key that is absent reads as 0, as a missing cv::FileNode does.  Returns {"calibration": Calibration, "camera_rgb": int,
    "width": int, "height": int, "fps": float, "th_depth": float, "extractor": {n_features, scale_factor, n_levels, ini_th_fast,
    min_th_fast}, "values": every key as text}."""
    vals = {}
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0]
            if line.startswith("%") or line.strip() in ("", "---"):
                continue
            m = _ENTRY.match(line)
            if m and m.group(2):
                vals[m.group(1)] = m.group(2).strip().strip('"')

    def num(key):
        return float(vals.get(key, "0"))

    def f32(key):
        return np.float32(num(key))

    def i32(key):   # (int) of a FileNode: an integer entry as written, a real one rounded
        return int(round(num(key)))

    cal = calibration(f32("Camera.fx"), f32("Camera.fy"), f32("Camera.cx"), f32("Camera.cy"), f32("Camera.k1"), f32("Camera.k2"),
                      f32("Camera.p1"), f32("Camera.p2"), f32("Camera.k3"), f32("Camera.bf"), f32("DepthMapFactor"))
    fps = float(f32("Camera.fps")) or 30.0
    return {
        "calibration": cal,
        "camera_rgb": i32("Camera.RGB"),
        "width": i32("Camera.width"),
        "height": i32("Camera.height"),
        "fps": fps,
        "th_depth": float(f32("ThDepth")),
        "extractor": {"n_features": i32("ORBextractor.nFeatures"), "scale_factor": float(f32("ORBextractor.scaleFactor")),
                      "n_levels": i32("ORBextractor.nLevels"), "ini_th_fast": i32("ORBextractor.iniThFAST"),
                      "min_th_fast": i32("ORBextractor.minThFAST")},
        "values": vals,
    }


_MATRIX = re.compile(r"^[ \t]*([A-Za-z_][A-Za-z0-9_.]*)[ \t]*:[ \t]*!!opencv-matrix[ \t]*\n[ \t]*rows[ \t]*:[ \t]*(\d+)[ \t]*\n"
                     r"[ \t]*cols[ \t]*:[ \t]*(\d+)[ \t]*\n[ \t]*dt[ \t]*:[ \t]*(\w+)[ \t]*\n[ \t]*data[ \t]*:[ \t]*\[([^\]]*)\]", re.M)
_RECT_SHAPES = {"K": (3, 3), "D": (1, 5), "R": (3, 3), "P": (3, 4)}


def read_stereo_rectification(path: str) -> dict:
    """The rectification entries of a stereo settings file (Source/Examples/Stereo/EuRoC.yaml) without OpenCV: LEFT. / RIGHT. K, D, R,
    P -- `!!opencv-matrix` blocks of rows, cols, dt and data (`data:[` or `data: [`, possibly over several lines) -- and LEFT. /
    RIGHT. height / width.  Raises ValueError where the reference's driver stops with "Calibration parameters to rectify stereo are
    missing" (Source/Examples/Stereo/stereo_euroc.cc:98-104): a matrix that is absent or empty, or a size of 0; and for a matrix of
    another shape than 3 x 3 (K, R), 1 x 5 (D: k1 k2 p1 p2 k3, no further coefficients) and 3 x 4 (P).
    Returns {"LEFT": {"K", "D", "R", "P": float64 arrays, "width", "height"}, "RIGHT": {...}}."""
    with open(path) as f:
        text = "\n".join(line.split("#", 1)[0].rstrip() for line in f.read().splitlines())
    mats = {}
    for m in _MATRIX.finditer(text):
        rows, cols = int(m.group(2)), int(m.group(3))
        data = [float(v) for v in m.group(5).replace("\n", " ").split(",") if v.strip()]
        if len(data) != rows * cols:
            raise ValueError(f"{path}: {m.group(1)} holds {len(data)} values for {rows} x {cols}")
        mats[m.group(1)] = np.array(data, np.float64).reshape(rows, cols)
    sizes = {}
    for line in text.splitlines():
        e = _ENTRY.match(line)
        if e and e.group(1) in ("LEFT.height", "LEFT.width", "RIGHT.height", "RIGHT.width") and e.group(2):
            sizes[e.group(1)] = int(round(float(e.group(2))))
    out = {}
    for eye in ("LEFT", "RIGHT"):
        cam = {}
        for name, shape in _RECT_SHAPES.items():
            a = mats.get(f"{eye}.{name}")
            if a is None or a.size == 0:
                raise ValueError(f"{path}: calibration parameters to rectify stereo are missing ({eye}.{name})")
            if a.shape != shape and not (name == "D" and a.shape == (5, 1)):
                raise ValueError(f"{path}: {eye}.{name} is {a.shape[0]} x {a.shape[1]}, expected {shape[0]} x {shape[1]}")
            cam[name] = a.reshape(shape)
        for side in ("width", "height"):
            cam[side] = sizes.get(f"{eye}.{side}", 0)
            if cam[side] == 0:
                raise ValueError(f"{path}: calibration parameters to rectify stereo are missing ({eye}.{side})")
        out[eye] = cam
    return out
