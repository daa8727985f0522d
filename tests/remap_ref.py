"""An independent numpy model of the stereo rectification's two definitions (include/orbgpu.h): cv::remap for 8-bit
one-channel images with CV_32FC1 maps, INTER_LINEAR and BORDER_CONSTANT 0 (OpenCV 3.2 remapBilinear's fixed point), and
cv::initUndistortRectifyMap with CV_32F maps.  Integer arithmetic is int64, the map builder's is float64 in the stated
order with np.add.accumulate for the sequential column sums.  Shared by the CPU and the GPU tests."""
import numpy as np

INT_MIN = -(1 << 31)


def fixed(m):
    """cvtss2si(m * 32.0f): float32 product, to nearest even, INT_MIN for NaN, +-inf and anything outside int."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(m, np.float32) * np.float32(32.0)
        bad = ~np.isfinite(p) | (p >= np.float32(2147483648.0)) | (p < np.float32(-2147483648.0))
        r = np.rint(np.where(bad, np.float32(0), p).astype(np.float64)).astype(np.int64)
    r[bad] = INT_MIN
    return r


def taps(map_x, map_y):
    """(ix, iy, fx, fy) as int64 arrays: the corner saturated to short, the 5-bit fractions."""
    sx, sy = fixed(map_x), fixed(map_y)
    ix, iy = np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767)
    return ix, iy, sx & 31, sy & 31


def _read(src, x, y):
    h, w = src.shape
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    if src.size == 0:
        return np.zeros(x.shape, np.int64)
    v = src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
    return np.where(inside, v, 0)


def remap(src, map_x, map_y):
    """The destination (the maps' shape) of remap(src, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, 0)."""
    src = np.asarray(src, np.uint8)
    ix, iy, fx, fy = taps(map_x, map_y)
    w00, w01, w10, w11 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32
    assert (w00 + w01 + w10 + w11 == 32768).all()
    acc = (w00 * _read(src, ix, iy) + w01 * _read(src, ix + 1, iy) + w10 * _read(src, ix, iy + 1) +
           w11 * _read(src, ix + 1, iy + 1) + 16384) >> 15
    assert acc.min(initial=0) >= 0 and acc.max(initial=0) <= 255
    return acc.astype(np.uint8)


def rectify_maps(K, D, R, P33, w, h):
    """initUndistortRectifyMap(K, D, R, P33, (w, h), CV_32F): (map_x, map_y) float32 of shape (h, w); None if P33 * R is
    singular.  Every operation is one float64 operation in the order the header states."""
    f64 = np.float64
    K, R, P = (np.asarray(a, f64).reshape(3, 3) for a in (K, R, P33))
    D = [f64(v) for v in np.asarray(D, f64).ravel()]
    assert len(D) in (4, 5, 8)
    k1, k2, p1, p2 = D[:4]
    k3 = D[4] if len(D) >= 5 else f64(0)
    k4, k5, k6 = D[5:8] if len(D) == 8 else (f64(0),) * 3
    A = np.zeros((3, 3), f64)
    for i in range(3):
        for j in range(3):
            s = P[i, 0] * R[0, j]
            s = s + P[i, 1] * R[1, j]
            s = s + P[i, 2] * R[2, j]
            A[i, j] = s
    a = A.ravel()
    det = a[0] * (a[4] * a[8] - a[7] * a[5]) - a[1] * (a[3] * a[8] - a[6] * a[5]) + a[2] * (a[3] * a[7] - a[6] * a[4])
    if det == 0 or not np.isfinite(det):
        return None
    d = f64(1.0) / det
    ir = [(a[4] * a[8] - a[5] * a[7]) * d, (a[2] * a[7] - a[1] * a[8]) * d, (a[1] * a[5] - a[2] * a[4]) * d,
          (a[5] * a[6] - a[3] * a[8]) * d, (a[0] * a[8] - a[2] * a[6]) * d, (a[2] * a[3] - a[0] * a[5]) * d,
          (a[3] * a[7] - a[4] * a[6]) * d, (a[1] * a[6] - a[0] * a[7]) * d, (a[0] * a[4] - a[1] * a[3]) * d]
    rows = np.arange(h, dtype=f64)

    def sweep(per_row, start, step):
        """start + i * per_row in column 0, then + step per column, summed left to right."""
        m = np.full((h, w), step, f64)
        m[:, 0] = rows * per_row + start
        return np.add.accumulate(m, axis=1)

    _x, _y, _w = sweep(ir[1], ir[2], ir[0]), sweep(ir[4], ir[5], ir[3]), sweep(ir[7], ir[8], ir[6])
    with np.errstate(all="ignore"):
        wi = f64(1.0) / _w
        x, y = _x * wi, _y * wi
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, f64(2) * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + f64(2) * x2)
        yd = y * kr + p1 * (r2 + f64(2) * y2) + p2 * _2xy
        return (K[0, 0] * xd + K[0, 2]).astype(np.float32), (K[1, 1] * yd + K[1, 2]).astype(np.float32)


def all_fractions_maps(x0=3, y0=2):
    """32 x 32 maps whose pixel (y, x) has fractions (fy, fx) = (y, x): all 1,024 pairs, each once."""
    g = np.arange(32, dtype=np.float32) / np.float32(32)
    return np.tile(np.float32(x0) + g, (32, 1)), np.tile((np.float32(y0) + g)[:, None], (1, 32))


def random_maps(dw, dh, sw, sh, seed):
    """A smooth map from the destination into the source (a mild shear and barrel) with a tenth of its pixels thrown
    outside: beyond each of the four sides, across the corners, and to positions neither int nor short holds."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(dh, dtype=np.float64), np.arange(dw, dtype=np.float64), indexing="ij")
    u, v = xx / max(dw - 1, 1) - 0.5, yy / max(dh - 1, 1) - 0.5
    r2 = u * u + v * v
    mx = ((u * (1 + 0.2 * r2) + 0.03 * v + 0.5) * (sw - 1) + rng.uniform(-0.4, 0.4, (dh, dw))).astype(np.float32)
    my = ((v * (1 - 0.15 * r2) - 0.02 * u + 0.5) * (sh - 1) + rng.uniform(-0.4, 0.4, (dh, dw))).astype(np.float32)
    out = np.flatnonzero(rng.random(dw * dh) < 0.1)
    far = [(-0.75, None), (sw - 0.25, None), (None, -0.75), (None, sh - 0.25), (-1.5, -1.5), (sw + 0.5, -0.5),
           (-0.5, sh + 0.5), (sw + 3.0, sh + 3.0), (4e4, None), (None, -4e4), (1e30, None), (np.nan, None),
           (None, np.inf), (-np.inf, np.nan)]
    for n, i in enumerate(out):
        fx, fy = far[n % len(far)]
        if fx is not None:
            mx.flat[i] = fx
        if fy is not None:
            my.flat[i] = fy
    return mx, my


# A EuRoC-like calibration (a 752 x 480 camera with a barrel distortion, a rectifying rotation of half a degree and a
# slightly longer rectified focal length; the numbers are this test's own), nine doubles row-major as a YAML gives them
EUROC_K = [460.0, 0.0, 368.5, 0.0, 458.25, 249.0, 0.0, 0.0, 1.0]
EUROC_D = [-0.28, 0.074, 0.0002, 1.8e-05, 0.0]
EUROC_P33 = [436.0, 0.0, 366.25, 0.0, 436.0, 251.5, 0.0, 0.0, 1.0]


def _rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return [float(v) for v in (Rz @ Ry @ Rx).ravel()]


EUROC_R = _rotation(0.007, 0.008, -0.0014)


def small_calibration(w, h, ncoef):
    """The EuRoC calibration scaled to a w x h image, with 4, 5 or 8 coefficients."""
    s = w / 752.0
    K = [EUROC_K[0] * s, 0.0, EUROC_K[2] * s, 0.0, EUROC_K[4] * s, EUROC_K[5] * s, 0.0, 0.0, 1.0]
    P = [EUROC_P33[0] * s, 0.0, EUROC_P33[2] * s, 0.0, EUROC_P33[4] * s, EUROC_P33[5] * s, 0.0, 0.0, 1.0]
    D = (EUROC_D[:4] + [0.011, 0.002, -0.003, 0.0007])[:ncoef]
    return K, D, EUROC_R, P


def raw_pair(orbgpu, w, h, idx):
    """A rectified synthetic pair (left, synth_stereo_right(left)), the rectification maps of a mildly distorted
    EuRoC-like stereo rig scaled to w x h, and the raw pair: the rectified images pushed through the approximate
    inverse of each map, so that rectifying the raw images gives textured, matchable images again."""
    from orbgpu.synth import synth_frame, synth_stereo_right
    left = synth_frame(w, h, idx)
    right = synth_stereo_right(left, idx, max_disp=24)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    out = []
    for eye, img in enumerate((left, right)):
        K, D, R, P = small_calibration(w, h, 5 if eye == 0 else 4)
        if eye == 1:
            R = list(np.reshape(R, (3, 3)).T.ravel())
        mx, my = orbgpu.rectify_maps_host(K, D, R, P, (w, h))
        raw = orbgpu.remap_host(img, (xx - (mx - xx)).astype(np.float32), (yy - (my - yy)).astype(np.float32))
        out.append((raw, mx, my))
    return out
