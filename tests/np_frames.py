"""Second reading of the per-keypoint tail of Frame::Frame in numpy, written from the reference and OpenCV's generic path rather than
from csrc/frame_internal.h: every operation is a separate float64 / float32 ufunc call, so each one rounds.

    cv::undistortPoints(pts, pts, mK, mDistCoef, cv::Mat(), mK)   OpenCV 4.5.4-4.6 cvUndistortPointsInternal: double, five iterations
                                                                   (COUNT only), R = I, P = K, k[5..11] = 0
    Frame::UndistortKeyPoints      L/src/Frame.cc:419-445
    Frame::ComputeImageBounds      L/src/Frame.cc:447-476
    Frame::ComputeStereoFromRGBD   L/src/Frame.cc:648-666, on the map Tracking::GrabImageRGBD scales (L/src/Tracking.cc:210-211)
"""
from __future__ import annotations

import numpy as np

f64, f32 = np.float64, np.float32


def undistort(cal, xy, report=False):
    """(n, 2) float32 points -> (n, 2) float32 undistorted points (and, report=True, the mask of points that left by icdist < 0).
    The generic loop with its zero terms written out: they are exact, so this is the reference's arithmetic term by term."""
    pts = np.asarray(xy, f32).reshape(-1, 2)
    u, v = pts[:, 0].astype(f64), pts[:, 1].astype(f64)
    fx, fy, cx, cy = (f64(f32(getattr(cal, k))) for k in ("fx", "fy", "cx", "cy"))
    k = [f64(f32(getattr(cal, n))) for n in ("k1", "k2", "p1", "p2", "k3")] + [f64(0)] * 7
    ifx, ify = f64(1) / fx, f64(1) / fy
    x = (u - cx) * ifx
    y = (v - cy) * ify
    # identity tilt: invMatTilt * (x, y, 1), invProj = 1 / 1
    x0 = x = f64(1) * (x * f64(1) + y * f64(0) + f64(0))
    y0 = y = f64(1) * (x * f64(0) + y * f64(1) + f64(0))
    active = np.ones(len(u), bool)
    neg = np.zeros(len(u), bool)
    with np.errstate(all="ignore"):
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            brk = active & (icdist < 0)
            x = np.where(brk, (u - cx) * ifx, x)
            y = np.where(brk, (v - cy) * ify, y)
            neg |= brk
            active &= ~brk
            deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = np.where(active, (x0 - deltaX) * icdist, x)
            y = np.where(active, (y0 - deltaY) * icdist, y)
        # RR = K * I
        xx = fx * x + f64(0) * y + cx
        yy = f64(0) * x + fy * y + cy
        ww = f64(1) / (f64(0) * x + f64(0) * y + f64(1))
    out = np.stack([(xx * ww).astype(f32), (yy * ww).astype(f32)], axis=1)
    return (out, neg) if report else out


def keys_un(cal, kps):
    """mvKeysUn: pt undistorted, every other field copied; mvKeys itself when k1 == 0 (Frame.cc:420-423)."""
    out = np.array(kps, copy=True)
    if f32(cal.k1) == 0:
        return out
    xy = undistort(cal, np.stack([kps["x"], kps["y"]], axis=1))
    out["x"], out["y"] = xy[:, 0], xy[:, 1]
    return out


def image_bounds(cal, w, h):
    """(mnMinX, mnMaxX, mnMinY, mnMaxY) of Frame::ComputeImageBounds."""
    if f32(cal.k1) == 0:
        return f32(0), f32(w), f32(0), f32(h)
    c = undistort(cal, np.array([[0, 0], [w, 0], [0, h], [w, h]], f32))
    mn = lambda a, b: b if b < a else a   # std::min
    mx = lambda a, b: b if a < b else a   # std::max
    return mn(c[0, 0], c[2, 0]), mx(c[1, 0], c[3, 0]), mn(c[0, 1], c[1, 1]), mx(c[2, 1], c[3, 1])


def depth_map(cal, raw):
    """GrabImageRGBD's convertTo: a 16-bit map always becomes (float)raw * factor; a float map only when |factor - 1| > 1e-5."""
    fac = f32(cal.depth_factor)
    if raw.dtype == np.uint16:
        return raw.astype(f32) * fac
    if float(np.abs(fac - f32(1))) > 1e-5:
        return raw.astype(f32) * fac
    return raw.astype(f32)


def rgbd_stereo(cal, kps, kpu, depth):
    """ComputeStereoFromRGBD on the converted float map `depth`: d = imDepth.at<float>((int)y, (int)x) of the DISTORTED keypoint;
    d > 0 -> mvDepth = d, mvuRight = kpU.x - mbf / d; otherwise -1, -1.  Truncated coordinates outside the map: no depth.
    Returns (u_right, depth, count)."""
    h, w = depth.shape
    x, y = kps["x"].astype(f32), kps["y"].astype(f32)
    inside = (x > -1) & (x < w) & (y > -1) & (y < h)
    xi = np.where(inside, np.trunc(np.where(inside, x, 0)), 0).astype(np.int64)
    yi = np.where(inside, np.trunc(np.where(inside, y, 0)), 0).astype(np.int64)
    d = np.where(inside, depth[yi, xi], f32(0)).astype(f32)
    has = d > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ur = np.where(has, kpu["x"].astype(f32) - f32(cal.mbf) / np.where(has, d, f32(1)), f32(-1)).astype(f32)
    dep = np.where(has, d, f32(-1)).astype(f32)
    return ur, dep, int(has.sum())


def distort(cal, xy_un):
    """Forward Brown-Conrady model in float64 (independent of the undistortion loop): pixel -> distorted pixel."""
    p = np.asarray(xy_un, f64).reshape(-1, 2)
    fx, fy, cx, cy = (float(getattr(cal, k)) for k in ("fx", "fy", "cx", "cy"))
    k1, k2, p1, p2, k3 = (float(getattr(cal, k)) for k in ("k1", "k2", "p1", "p2", "k3"))
    x, y = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * fx + cx, yd * fy + cy], axis=1)


# The cameras of the tests: the reference's settings files (Source/Examples/RGB-D/TUM1.yaml, TUM2.yaml, Monocular/TUM1.yaml,
# Monocular/EuRoC.yaml) and three made-up ones: k3 = 0 with k2 != 0, a strong barrel camera whose loop takes the icdist < 0 exit, and a
# "steep" one whose corners move inward far more than the edge midpoints.  With TUM1 a keypoint would have to lie within ~6 px of the
# image edge to undistort outside the bounds (the extractor keeps ~16 px away); with the steep camera extracted keypoints do.
# (fx, fy, cx, cy, k1, k2, p1, p2, k3, bf, DepthMapFactor), image size
CAMERAS = {
    "tum1_rgbd": ((517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0, 5000.0), (640, 480)),
    "tum2_rgbd": ((520.908620, 521.007327, 325.141442, 249.701764, 0.231222, -0.784899, -0.003257, -0.000105, 0.917205, 40.0, 5208.0), (640, 480)),
    "tum1_mono": ((517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 0.0, 0.0), (640, 480)),
    "euroc_mono": ((458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0, 0.0, 0.0), (752, 480)),
    "k3_zero": ((500.0, 505.0, 320.5, 240.25, 0.12, -0.21, 0.001, -0.0007, 0.0, 40.0, 1000.0), (640, 480)),
    "strong": ((400.0, 400.0, 320.0, 240.0, -2.0, 0.5, 0.0, 0.0, 0.0, 40.0, 5000.0), (640, 480)),
    "steep": ((517.306408, 516.469215, 318.643040, 255.313989, -0.3, 0.0, 0.001, -0.002, 2.5, 40.0, 5000.0), (640, 480)),
}
TUM3 = ((535.4, 539.2, 320.1, 247.6, 0.0, 0.0, 0.0, 0.0, 0.0, 40.0, 5000.0), (640, 480))


def camera(name):
    """(Calibration, (w, h)) of a CAMERAS entry."""
    from refactored_orb_slam2_amd.camera import calibration
    vals, wh = CAMERAS[name] if name in CAMERAS else TUM3
    return calibration(*vals), wh


def dense_points(w, h, step=7.3, margin=40.0):
    """A dense grid over and beyond the image with fractional coordinates, plus the corners and edge midpoints."""
    xs = np.arange(-margin, w + margin, step, dtype=np.float64)
    ys = np.arange(-margin, h + margin, step * 0.91, dtype=np.float64)
    g = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    extra = [[0, 0], [w, 0], [0, h], [w, h], [w / 2, 0], [0, h / 2], [w, h / 2], [w / 2, h], [w - 0.5, h - 0.5], [0.25, 0.75]]
    return np.concatenate([g, np.array(extra, np.float64)]).astype(f32)
