"""Inputs of the resident map point tests, generated on the CPU from fixed seeds: a camera, the planted points (one
per branch and per side of each comparison of Frame::isInFrustum, Fuse's projection and PredictScale), a random shell
of points around the camera, and map points back-projected from a frame's features (so that the searches find them).
tests/test_frustum_ref.py checks the planted decisions on frustum_ref; tests/test_gpu_points.py runs everything on the
GPU against frustum_ref."""
import functools

import numpy as np

import frustum_ref as ref

f32, f64 = np.float32, np.float64
NLEVELS = 8
SCALE = np.ones(NLEVELS, f32)
for _i in range(1, NLEVELS):
    SCALE[_i] = SCALE[_i - 1] * f32(1.2)                         # ORBextractor.cc:431-437
LSF = ref.logf(f32(1.2))                                          # mfLogScaleFactor = log(mfScaleFactor)
IMAGE = (0.0, 640.0, 0.0, 480.0)

# the planted points' camera: the identity pose, so Pc = P exactly, and fx * 0.625 = cx = 320 puts u on a bound
PLANT_CAM = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), Ow=np.zeros(3, f32), fx=512.0, fy=512.0, cx=320.0,
                 cy=240.0, mbf=40.0, bounds=IMAGE, scale_factors=SCALE, log_scale_factor=LSF)


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def down(x):
    return np.nextafter(f32(x), f32(-np.inf))


def rot(axis, angle):
    """Rodrigues rotation as float32 (its orthogonality is as good as a SLAM pose's: the tests need no more)."""
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(f32)


def make_camera(seed, bounds=IMAGE):
    """A general pose: Ow = -Rcw^T tcw in float32, as KeyFrame::SetPose computes it (its last bits do not matter here:
    Ow is an input of the projection)."""
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), rng.uniform(0.2, 1.2))
    t = rng.uniform(-2, 2, 3).astype(f32)
    Ow = (-(R.T.astype(f64) @ t.astype(f64))).astype(f32)
    return dict(Rcw=R, tcw=t, Ow=Ow, fx=517.3, fy=516.5, cx=318.6, cy=255.3, mbf=40.0, bounds=bounds,
                scale_factors=SCALE, log_scale_factor=LSF)


def cam_struct(orbgpu, cam):
    return orbgpu.camera(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"],
                         cam["bounds"], cam["scale_factors"], cam["log_scale_factor"])


@functools.lru_cache(maxsize=None)
def thresholds():
    return ref.level_thresholds(LSF, NLEVELS)


def _gate_value(factor, dist, above):
    """A raw distance d with float32(factor * d) == dist (above = False) or the smallest one whose product exceeds
    dist (above = True)."""
    d = f32(f32(dist) / f32(factor))
    for _ in range(8):
        d = down(d)
    last_equal = None
    for _ in range(32):
        p = f32(f32(factor) * d)
        if p == f32(dist):
            last_equal = d
        if p > f32(dist):
            assert last_equal is not None
            return d if above else last_equal
        d = up(d)
    raise AssertionError("no raw distance reaches the gate")


@functools.lru_cache(maxsize=None)
def planted():
    """(name, pos, normal, min_dist, max_dist, verdict FRAME, verdict FUSE, level or None, radius factor or None) with
    view_cos_limit = 0.5.  The radius factor is FRAME's r0 before th: 2.5 or 4.0."""
    V, D, B, S, A, N = ref.VISIBLE, ref.DEPTH, ref.BOUNDS, ref.DISTANCE, ref.ANGLE, ref.NOT_FINITE
    z = (0.0, 0.0, 1.0)
    T = thresholds()
    P = []

    def add(name, pos, normal=z, lo=0.0, hi=100.0, frame=V, fuse=V, level=None, r0=None):
        P.append((name, np.array(pos, f32), np.array(normal, f32), f32(lo), f32(hi), frame, fuse, level, r0))

    # depth: PcZ just below 0 / exactly 0 (u = fma(0, inf, cx) is NaN: FRAME's comparisons all pass, IsInImage fails)
    add("z_below_0", (0, 0, -1e-45), frame=D, fuse=D)
    add("z_0_x_0", (0, 0, 0), hi=1.0, frame=N, fuse=B)
    add("z_0_x_1", (1, 0, 0), frame=B, fuse=B)                       # u = +inf
    # bounds: u == max_x (FRAME keeps: u > max_x; FUSE rejects: u < max_x), u == min_x (both keep), one float outside
    add("u_max", (0.625, 0, 1), normal=(0.625, 0, 1), fuse=B)
    add("u_above_max", (0.625 + 2.0 ** -20, 0, 1), normal=(0.625, 0, 1), frame=B, fuse=B)   # u = 640 + 2^-11 exactly
    add("u_min", (-0.625, 0, 1), normal=(-0.625, 0, 1))
    add("u_below_min", (down(-0.625), 0, 1), normal=(-0.625, 0, 1), frame=B, fuse=B)
    add("v_max", (0, 0.46875, 1), normal=(0, 0.46875, 1), fuse=B)    # 512 * 0.46875 + 240 = 480
    add("v_min", (0, -0.46875, 1), normal=(0, -0.46875, 1))
    add("v_below_min", (0, down(-0.46875), 1), normal=(0, -0.46875, 1), frame=B, fuse=B)
    # distance: dist == 0.8f * min_dist and == 1.2f * max_dist are kept, the next raw distance is not
    add("dist_at_min", (0, 0, 4), lo=_gate_value(0.8, 4.0, False), hi=100.0)
    add("dist_below_min", (0, 0, 4), lo=_gate_value(0.8, 4.0, True), hi=100.0, frame=S, fuse=S)
    add("dist_at_max", (0, 0, 6), hi=_gate_value(1.2, 6.0, False))
    add("dist_above_max", (0, 0, 6), hi=down(_first_equal(1.2, 6.0)), frame=S, fuse=S)
    # angle: view_cos == 0.5 / dot == 0.5 * dist are kept, one float less is not
    add("cos_at_limit", (0, 0, 4), normal=(0, 0, 0.5))
    add("cos_below_limit", (0, 0, 4), normal=(0, 0, down(0.5)), frame=A, fuse=A)
    # radius: view_cos on both sides of the double 0.998
    add("cos_above_0998", (0, 0, 1), normal=(0, 0, f32(0.998)), hi=1.0, r0=2.5)
    add("cos_below_0998", (0, 0, 1), normal=(0, 0, down(f32(0.998))), hi=1.0, r0=4.0)
    # level: a ratio one float below and at a threshold (dist = 1: ratio = max_dist), and the clamps
    for k in (0, 3, NLEVELS - 2):
        add("ratio_at_T%d" % k, (0, 0, 1), hi=T[k], level=k + 1)
        add("ratio_below_T%d" % k, (0, 0, 1), hi=down(T[k]), level=k)
    add("level_clamp_0", (0, 0, 1.125), hi=1.0, level=0)            # ratio < 1: ceil < 0
    add("level_clamp_top", (0, 0, 1), hi=100.0, level=NLEVELS - 1)
    return tuple(P)


def _first_equal(factor, dist):
    """The smallest raw distance d with float32(factor * d) == dist."""
    d = _gate_value(factor, dist, False)
    while f32(f32(factor) * down(d)) == f32(dist):
        d = down(d)
    return d


def arrays(points):
    """(pos, normal, min_dist, max_dist) arrays of planted()-style tuples."""
    return (np.stack([p[1] for p in points]), np.stack([p[2] for p in points]),
            np.array([p[3] for p in points], f32), np.array([p[4] for p in points], f32))


def random_points(seed, n, cam):
    """Points in a shell around the camera: a sixth behind it, the others spread over a window a quarter wider than the
    image; normals around the viewing ray; distance limits drawn around each point's true distance."""
    rng = np.random.default_rng(seed)
    R, t = np.asarray(cam["Rcw"], f64), np.asarray(cam["tcw"], f64)
    z = rng.uniform(1.0, 10.0, n)
    u = rng.uniform(-80, 720, n)
    v = rng.uniform(-60, 540, n)
    Pc = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], 1)
    behind = rng.random(n) < 1 / 6
    Pc[behind] *= -1
    pos = ((Pc - t) @ R).astype(f32)                                # R^T (Pc - t)
    PO = pos.astype(f64) - np.asarray(cam["Ow"], f64)
    d = np.linalg.norm(PO, axis=1)
    nr = PO / d[:, None] + rng.normal(scale=0.9, size=(n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(f32)
    lo = (d * rng.uniform(0.4, 1.5, n)).astype(f32)
    hi = (d * np.exp(rng.uniform(-0.5, 2.0, n))).astype(f32)
    return pos, nr, lo, hi


def points_on_features(seed, cam, kps, desc, nflip=6, frac_turned=0.15):
    """One map point per keypoint: back-projected at a random depth through cam, so that it projects onto the
    keypoint (within float error); its descriptor is the feature's with up to nflip bits changed; its normal looks at
    the camera (a share of frac_turned looks away: rejected by the angle test); max_dist puts the predicted level at
    the keypoint's octave or next to it."""
    rng = np.random.default_rng(seed)
    n = len(kps)
    R, t = np.asarray(cam["Rcw"], f64), np.asarray(cam["tcw"], f64)
    z = rng.uniform(2.0, 9.0, n)
    Pc = np.stack([(kps["x"].astype(f64) - cam["cx"]) / cam["fx"] * z, (kps["y"].astype(f64) - cam["cy"]) / cam["fy"] * z,
                   z], 1)
    pos = ((Pc - t) @ R).astype(f32)
    PO = pos.astype(f64) - np.asarray(cam["Ow"], f64)
    d = np.linalg.norm(PO, axis=1)
    nr = PO / d[:, None] + rng.normal(scale=0.2, size=(n, 3))
    turned = rng.random(n) < frac_turned
    nr[turned] *= -1
    nr = (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(f32)
    level = np.clip(kps["octave"] + rng.integers(-1, 2, n), 0, NLEVELS - 1)
    hi = (d * 1.2 ** (level - 0.5)).astype(f32)                     # ceil(log(ratio) / log 1.2) = level
    lo = (d * rng.uniform(0.3, 1.3, n)).astype(f32)
    out = np.ascontiguousarray(desc).copy()
    for i in range(n):
        for b in rng.choice(256, int(rng.integers(0, nflip + 1)), replace=False):
            out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return pos, nr, lo, hi, out


def visible_queries(orbgpu, rec):
    """The orb_proj_query array of the visible records, as include/orbgpu.h maps SearchByProjection(Frame&,
    vector<MapPoint*>, th) and Fuse: levels (level - 1, level), ur_tol = r, blocks = 1; and their positions."""
    vis = np.flatnonzero(rec["verdict"] == 0)
    q = orbgpu.proj_queries(rec["u"][vis], rec["v"][vis], rec["r"][vis], rec["level"][vis], rec["ur"][vis])
    q["ur_tol"] = rec["r"][vis]
    return q, vis
