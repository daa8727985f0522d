"""Test-side restatement of the reference's map point projection, in float32 / float64 scalars:

  is_in_frustum     Frame::isInFrustum (src/Frame.cc:436-492) with the search radius of SearchByProjection(Frame&,
                    vector<MapPoint*>, th) (src/ORBmatcher.cc:63-69, RadiusByViewingCos :131-137)
  fuse_projection   the projection loop of Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:852-890)
                    with KeyFrame::IsInImage (src/KeyFrame.cc:627-630)
  predict_scale     MapPoint::PredictScale (src/MapPoint.cc:385-417), with the host libm's logf through ctypes

A camera is a dict: Rcw (3x3), tcw, Ow, fx, fy, cx, cy, mbf, bounds (mnMinX, mnMaxX, mnMinY, mnMaxY), scale_factors
(mvScaleFactors), log_scale_factor (mfLogScaleFactor).  A point is (pos, normal, min_dist, max_dist) with the raw
mfMinDistance / mfMaxDistance; GetMinDistanceInvariance / GetMaxDistanceInvariance (MapPoint.cc:373-383) are
0.8f * mfMinDistance and 1.2f * mfMaxDistance.

cv::Mat arithmetic: Rcw * P + tcw is OpenCV's gemm, float products accumulated in double left to right, t added in
double, rounded once (the model of tests/cpp/cv_api/opencv2/core/core.hpp); cv::norm and Mat::dot accumulate in
double.  The scalar float lines are in the contracted forms of the reference's -O3 -march=native build
(tools/frustum_flags_probe.cpp, tests/test_frustum_pin.py), with the exact float32 fmaf of kf_projection_ref.

Every function returns a record (dict) with the fields of orb_point_proj: what the reference had computed when it
returned; the other fields 0 and level -1.  verdict: 0 visible, 1 depth, 2 bounds, 3 distance, 4 angle, and 5, the
one decided deviation: every test passed but u, v, ur or r is not finite (the reference goes on into casts of such
values, which are undefined).  A ratio that is not finite gives level 0 (what the x86 cast of its ceil yields)."""
import ctypes
import ctypes.util
import math

import numpy as np

from kf_projection_ref import fmaf

f32, f64 = np.float32, np.float64
VISIBLE, DEPTH, BOUNDS, DISTANCE, ANGLE, NOT_FINITE = range(6)
FIELDS = ("u", "v", "ur", "invz", "dist", "view_cos", "r", "level", "verdict")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    return f32(_libm.logf(float(f32(x))))


def _fma(a, b, c):
    """float32 fma that also takes the non-finite operands the planted points produce."""
    a, b, c = f32(a), f32(b), f32(c)
    if np.isfinite(a) and np.isfinite(b) and np.isfinite(c):
        return fmaf(a, b, c)
    with np.errstate(all="ignore"):
        return f32(f64(a) * f64(b) + f64(c))     # inf / nan propagate as in hardware (no finite rounding is involved)


def predict_scale(max_dist, dist, log_scale_factor, nlevels):
    """MapPoint.cc:402-417: ratio = mfMaxDistance / currentDist; nScale = ceil(log(ratio) / mfLogScaleFactor), clamped."""
    with np.errstate(all="ignore"):
        ratio = f32(f32(max_dist) / f32(dist))
    return level_of_ratio(ratio, log_scale_factor, nlevels)


def level_of_ratio(ratio, log_scale_factor, nlevels):
    ratio = f32(ratio)
    if not np.isfinite(ratio):
        return 0
    with np.errstate(all="ignore"):
        s = f32(np.ceil(f32(logf(ratio) / f32(log_scale_factor)))) if ratio > 0 else f32(np.nan)
    if not (s >= 0):           # nScale < 0, and the NaN of a negative ratio (its cast is INT_MIN on x86)
        return 0
    if s >= nlevels:
        return nlevels - 1
    return int(s)


def _gemm_row(R, P, t):
    s = (f64(f32(R[0])) * f64(f32(P[0])) + f64(f32(R[1])) * f64(f32(P[1]))) + f64(f32(R[2])) * f64(f32(P[2]))
    return f32(s + f64(f32(t)))


def _record():
    r = {k: f32(0.0) for k in FIELDS}
    r["level"], r["verdict"] = -1, VISIBLE
    return r


def _camera_space(cam, pos):
    R = np.asarray(cam["Rcw"], f32).reshape(3, 3)
    t = np.asarray(cam["tcw"], f32).ravel()
    P = np.asarray(pos, f32).ravel()
    return P, [_gemm_row(R[i], P, t[i]) for i in range(3)]


def _dist_and_dot(cam, P, normal):
    Ow, n = np.asarray(cam["Ow"], f32).ravel(), np.asarray(normal, f32).ravel()
    PO = [f32(P[i] - Ow[i]) for i in range(3)]
    n2 = (f64(PO[0]) * f64(PO[0]) + f64(PO[1]) * f64(PO[1])) + f64(PO[2]) * f64(PO[2])
    dist = f32(np.sqrt(n2))                                        # cv::norm: sqrt of the double sum
    dot = (f64(PO[0]) * f64(n[0]) + f64(PO[1]) * f64(n[1])) + f64(PO[2]) * f64(n[2])
    return dist, dot


def _finish(cam, rec, r0, max_dist):
    sf = np.asarray(cam["scale_factors"], f32)
    rec["level"] = predict_scale(max_dist, rec["dist"], cam["log_scale_factor"], len(sf))
    with np.errstate(all="ignore"):
        rec["r"] = f32(f32(r0) * sf[rec["level"]])
    if not all(np.isfinite(rec[k]) for k in ("u", "v", "ur", "r")):
        rec["verdict"] = NOT_FINITE
    return rec


def is_in_frustum(cam, pos, normal, min_dist, max_dist, view_cos_limit, th):
    rec = _record()
    P, (PcX, PcY, PcZ) = _camera_space(cam, pos)
    fx, fy, cx, cy, mbf = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy", "mbf"))
    min_x, max_x, min_y, max_y = (f32(b) for b in cam["bounds"])
    with np.errstate(all="ignore"):
        if PcZ < f32(0.0):                                          # :450
            rec["verdict"] = DEPTH
            return rec
        invz = f32(f32(1.0) / PcZ)                                  # :454
        rec["invz"] = invz
        rec["u"] = u = _fma(f32(fx * PcX), invz, cx)                # :455  fx*PcX*invz+cx
        rec["v"] = v = _fma(f32(fy * PcY), invz, cy)                # :456
        if u < min_x or u > max_x or v < min_y or v > max_y:        # :458-461
            rec["verdict"] = BOUNDS
            return rec
        dist, dot = _dist_and_dot(cam, P, normal)                   # :466-467
        rec["dist"] = dist
        if dist < f32(f32(0.8) * f32(min_dist)) or dist > f32(f32(1.2) * f32(max_dist)):   # :469
            rec["verdict"] = DISTANCE
            return rec
        view_cos = f32(dot / f64(dist))                             # :475  (double) dot / (double) dist, to float
        rec["view_cos"] = view_cos
        if view_cos < f32(view_cos_limit):                          # :477
            rec["verdict"] = ANGLE
            return rec
        rec["ur"] = _fma(-mbf, invz, u)                             # :486  u - mbf*invz
        r0 = f32(2.5) if f64(view_cos) > 0.998 else f32(4.0)        # ORBmatcher.cc:131-137
        if f32(th) != f32(1.0):                                     # :65-66
            r0 = f32(r0 * f32(th))
    return _finish(cam, rec, r0, max_dist)                          # Frame.cc:481, ORBmatcher.cc:68


def fuse_projection(cam, pos, normal, min_dist, max_dist, th):
    rec = _record()
    P, (PcX, PcY, PcZ) = _camera_space(cam, pos)
    fx, fy, cx, cy, mbf = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy", "mbf"))
    min_x, max_x, min_y, max_y = (f32(b) for b in cam["bounds"])
    with np.errstate(all="ignore"):
        if PcZ < f32(0.0):                                          # :856
            rec["verdict"] = DEPTH
            return rec
        invz = f32(f32(1.0) / PcZ)                                  # :859
        rec["invz"] = invz
        x, y = f32(PcX * invz), f32(PcY * invz)                     # :860-861
        rec["u"] = u = _fma(fx, x, cx)                              # :863
        rec["v"] = v = _fma(fy, y, cy)                              # :864
        if not (u >= min_x and u < max_x and v >= min_y and v < max_y):   # :867, KeyFrame.cc:627-630
            rec["verdict"] = BOUNDS
            return rec
        rec["ur"] = _fma(-mbf, invz, u)                             # :870
        dist, dot = _dist_and_dot(cam, P, normal)                   # :874-875
        rec["dist"] = dist
        if dist < f32(f32(0.8) * f32(min_dist)) or dist > f32(f32(1.2) * f32(max_dist)):   # :878
            rec["verdict"] = DISTANCE
            return rec
        if dot < 0.5 * f64(dist):                                   # :884
            rec["verdict"] = ANGLE
            return rec
    return _finish(cam, rec, f32(th), max_dist)                     # :887-890


def project(mode, cam, pos, normal, min_dist, max_dist, view_cos_limit=0.5, th=1.0):
    """Records for arrays of points: mode 0 = is_in_frustum, 1 = fuse_projection."""
    out = []
    for i in range(len(pos)):
        if mode == 0:
            out.append(is_in_frustum(cam, pos[i], normal[i], min_dist[i], max_dist[i], view_cos_limit, th))
        else:
            out.append(fuse_projection(cam, pos[i], normal[i], min_dist[i], max_dist[i], th))
    return out


def as_array(records, dtype):
    """The records as a structured array of the product's POINT_PROJ_DTYPE."""
    a = np.zeros(len(records), dtype)
    for i, r in enumerate(records):
        for k in FIELDS:
            a[k][i] = r[k]
    return a


def level_thresholds(log_scale_factor, nlevels):
    """T[k], k = 0 .. nlevels - 2: the smallest positive finite float32 r with ceilf(logf(r) / lsf) > k, by bisection
    over the float bit patterns (math.inf when there is none)."""
    lsf = f32(log_scale_factor)

    def val(b):
        return np.array([b], np.uint32).view(f32)[0]

    def above(b, k):
        return f32(np.ceil(f32(logf(val(b)) / lsf))) > k

    T = []
    for k in range(nlevels - 1):
        lo, hi = 1, 0x7F7FFFFF
        if not above(hi, k):
            T.append(f32(math.inf))
            continue
        if above(lo, k):
            T.append(val(lo))
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if above(mid, k):
                hi = mid
            else:
                lo = mid
        T.append(val(hi))
    return T
