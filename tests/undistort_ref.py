"""cv::fisheye::undistortPoints as Frame::UndistortKeyPoints / ComputeImageBounds call it (Frame.cc:571-660), restated
in scalar Python float64 (OpenCV 3.2 fisheye.cpp, x86-64 without FMA).  math.tan and math.sqrt per point:
the C library's, as the host twin's std::tan (numpy may dispatch a SIMD tan of its own).  Python floats are IEEE
doubles and an expression is evaluated left to right, one rounding per operation, which is the definition's order.

Shared by test_undistort_ref.py (the host twin against this restatement) and the GPU tests (their calibrations and
point sets)."""
import math
import struct

import numpy as np

# Examples/Monocular/fisheye.yaml (Camera.fx, fy, cx, cy, k1, k2, p1, p2: the fisheye model reads the four as k1..k4)
YAML = (348.5, 347.0, 480.0, 302.0, (-0.0488316, 0.000298406, -0.00591118, 0.00193258))
# mild: theta_d stays below 1.2 everywhere in 640 x 480 (the farthest corner is 400 px from the centre: 400 / 420)
MILD = (420.0, 418.0, 320.0, 240.0, (-0.02, 0.003, -0.0005, 0.0001))
# the principal point outside the image
OUTSIDE = (300.0, 310.0, -75.5, 610.25, (0.03, -0.004, 0.0007, -0.0002))
CALIBRATIONS = {"yaml": YAML, "mild": MILD, "outside": OUTSIDE}
# the principal point at the origin: floats a few 1e-6 px from it exist, so both sides of theta_d > 1e-8 are reachable
BRANCH = (350.0, 350.0, 0.0, 0.0, YAML[4])
IMAGE_SIZES = ((160, 120), (320, 240), (640, 480), (950, 400))

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)   # numeric_limits<float>::min(): the smallest positive normal float
HALF_PI = 3.1415926535897932384626433832795 / 2.0   # CV_PI / 2


def f32(v):
    return float(np.float32(v))


def calib32(cal):
    """The calibration as the floats the library receives."""
    fx, fy, cx, cy, k = cal
    return f32(fx), f32(fy), f32(cx), f32(cy), tuple(f32(v) for v in k)


def bits(v):
    """The float32 bit pattern a result is stored as: the double rounded to float, every NaN as 0x7FC00000."""
    if v != v:
        return 0x7FC00000
    with np.errstate(over="ignore"):
        return struct.unpack("<I", struct.pack("<f", np.float32(v)))[0]


def undistort_scale(cal, x, y):
    """(pw0, pw1, scale, took_iteration) of one point; x, y are float32 values."""
    fx, fy, cx, cy, k = calib32(cal)
    pw0 = (float(x) - cx) / fx
    pw1 = (float(y) - cy) / fy
    th_d = math.sqrt(pw0 * pw0 + pw1 * pw1)
    lo = -HALF_PI
    th_d = th_d if lo < th_d else lo            # std::max(-pi/2, th_d): (a < b) ? b : a
    th_d = HALF_PI if HALF_PI < th_d else th_d  # std::min(..., pi/2):  (b < a) ? b : a
    scale, iterate = 1.0, th_d > 1e-8
    if iterate:
        th = th_d
        for _ in range(10):
            t2 = th * th
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t6 * t2
            th = th_d / (1 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8)
        scale = math.tan(th) / th_d
    return pw0, pw1, scale, iterate


def undistort_point(cal, x, y):
    """The two float32 bit patterns of one undistorted point (not the identity path)."""
    fx, fy, cx, cy, _ = calib32(cal)
    pw0, pw1, scale, _ = undistort_scale(cal, x, y)
    pu0 = pw0 * scale
    pu1 = pw1 * scale
    pr0 = ((0 + fx * pu0) + 0 * pu1) + cx * 1
    pr1 = ((0 + 0 * pu0) + fy * pu1) + cy * 1
    pr2 = ((0 + 0 * pu0) + 0 * pu1) + 1 * 1
    return bits(pr0 / pr2), bits(pr1 / pr2)


def undistort_points(cal, xy):
    """(n, 2) float32 in, (n, 2) float32 out (compare as bit patterns: .view(np.uint32))."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    if calib32(cal)[4][0] == 0.0:   # Frame.cc:573: mvKeysUn = mvKeys
        return xy.copy()
    out = np.zeros(xy.shape, np.uint32)
    for i, (x, y) in enumerate(xy):
        out[i] = undistort_point(cal, x, y)
    return out.view(np.float32)


def image_bounds(cal, w, h):
    """(mnMinX, mnMaxX, mnMinY, mnMaxY) as float32 values (Frame.cc:605-660)."""
    if calib32(cal)[4][0] == 0.0:
        return np.array([0.0, w, 0.0, h], np.float32)
    un = undistort_points(cal, [(0, 0), (w, 0), (0, h), (w, h)])
    mnx, mxx, mny, mxy = np.float32(FLT_MAX), np.float32(FLT_MIN), np.float32(FLT_MAX), np.float32(FLT_MIN)
    for x, y in un:
        if x < mnx:
            mnx = x
        if x > mxx:
            mxx = x
        if y < mny:
            mny = y
        if y > mxy:
            mxy = y
    return np.array([mnx, mxx, mny, mxy], np.float32)


def seeded_points(cal, w, h, n, seed):
    """n float32 points: uniform over the image with a margin of a quarter of it on every side, and the special places
    (the principal point, points 3e-6 and 4e-6 px from it, the corners, far points that reach the pi/2 clip).  The
    two near points lie on the two sides of the theta_d > 1e-8 branch when the principal point is the origin and the
    focal length about 350 (BRANCH); around a principal point of some size no float lies that near."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, _ = calib32(cal)
    pts = np.stack([rng.uniform(-0.25 * w, 1.25 * w, n), rng.uniform(-0.25 * h, 1.25 * h, n)], 1).astype(np.float32)
    special = [(cx, cy), (cx + 3e-6, cy), (cx + 4e-6, cy), (cx, cy - 4e-6), (0, 0), (w, 0), (0, h), (w, h),
               (cx + 1.6 * fx, cy), (cx - 2.5 * fx, cy + 2.0 * fy), (cx + 1.5707 * fx, cy), (cx, cy + 40.0 * fy)]
    pts[:len(special)] = np.array(special, np.float32)[:n]
    return pts
