"""numpy restatements of the colour and RGB-D definitions (include/orbgpu.h), never the code under test:
cvtColor to gray as OpenCV 3.2's RGB2Gray<uchar> (x86-64, no IPP), and Frame::ComputeStereoFromRGBD (Frame.cc:839-860)
with GrabImageRGBD's convertTo folded in, every float step taken in np.float32.  Also the planted RGB-D case the host
and GPU tests share."""
import numpy as np

f32 = np.float32
COLOR_RGB, COLOR_BGR, COLOR_RGBA, COLOR_BGRA = 0, 1, 2, 3
DEPTH_U16, DEPTH_F32 = 0, 1
CHANNELS = {COLOR_RGB: 3, COLOR_BGR: 3, COLOR_RGBA: 4, COLOR_BGRA: 4}

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
               ("class_id", "<i4")])


def gray_rgb(r, g, b):
    """Y = (4899 R + 9617 G + 1868 B + 8192) >> 14 in exact integers."""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def to_gray(img, color):
    """img: (..., C) uint8 in the channel order `color` names; alpha ignored."""
    a = np.asarray(img)
    assert a.shape[-1] == CHANNELS[color]
    c0, c1, c2 = a[..., 0], a[..., 1], a[..., 2]
    return gray_rgb(c2, c1, c0) if color in (COLOR_BGR, COLOR_BGRA) else gray_rgb(c0, c1, c2)


def stereo_from_rgbd(depth_image, factor, kps, kps_un, mbf):
    """(uright, depth, nvalid, outside): the definition, with -1 / -1 for a keypoint whose truncated position is outside
    the image or not finite (outside[i] True: the host-array entry point refuses the whole call for such a keypoint)."""
    d_img = np.asarray(depth_image)
    h, w = d_img.shape
    factor, mbf = f32(factor), f32(mbf)
    n = len(kps)
    ur = np.full(n, -1, f32)
    dep = np.full(n, -1, f32)
    outside = np.zeros(n, bool)
    nvalid = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            x, y = f32(kps["x"][i]), f32(kps["y"][i])
            if not (np.isfinite(x) and np.isfinite(y)):
                outside[i] = True
                continue
            col, row = int(np.trunc(x)), int(np.trunc(y))   # Mat::at<float>(float, float): toward zero
            if not (0 <= col < w and 0 <= row < h):
                outside[i] = True
                continue
            d = f32(f32(d_img[row, col]) * factor)           # convertTo: float work type, one rounding
            if d > 0:
                nvalid += 1
                dep[i] = d
                q = f32(mbf / d)                             # the float division first
                ur[i] = f32(f32(kps_un["x"][i]) - q)
    return ur, dep, nvalid, outside


MAP_W, MAP_H = 16, 12
SPECIAL_F32 = [0.0, -0.0, -1.0, np.nan, np.inf, 1e-40, 2.5, 1234.5678, 3e-39, 65535.0, 1e30, -np.inf]
SPECIAL_U16 = [0, 1, 65535, 5000, 2, 40000, 12345, 3, 0, 1, 65535, 7]


def planted_map(kind, seed=5):
    """A MAP_H x MAP_W depth image of type `kind` ("u16" / "f32"): the special values in row 0 (column j holds special
    j), seeded values elsewhere with zeros sprinkled in."""
    rng = np.random.default_rng(seed)
    if kind == "u16":
        m = rng.integers(0, 65536, (MAP_H, MAP_W)).astype(np.uint16)
        m[rng.random((MAP_H, MAP_W)) < 0.2] = 0
        m[0, :len(SPECIAL_U16)] = SPECIAL_U16
    else:
        m = (rng.random((MAP_H, MAP_W)) * 20).astype(f32)
        m[rng.random((MAP_H, MAP_W)) < 0.2] = 0
        m[0, :len(SPECIAL_F32)] = np.array(SPECIAL_F32, f32)
    return m


def planted_keypoints(n, seed=9, with_outside=False):
    """n raw keypoints over the planted map and their 'undistorted' twins (x and y shifted, so that using the wrong
    array for the lookup or for uright shows).  The first 12 sit on the special values of row 0 at fractional
    positions (x = col + 0.999: column col, not col + 1; y in [0, 1)); number 12 is x = 10.999f exactly.  with_outside:
    the last two are outside the image (x = MAP_W) and not finite (NaN)."""
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KP)
    k.view(np.uint8).reshape(-1, 28)[:] = rng.integers(0, 256, (n, 28), dtype=np.uint8)
    col = rng.integers(0, MAP_W, n)
    row = rng.integers(0, MAP_H, n)
    frac = rng.choice(np.array([0.0, 0.25, 0.5, 0.999], f32), (n, 2))
    x = col.astype(f32) + frac[:, 0]
    y = row.astype(f32) + frac[:, 1]
    ns = min(n, 12)
    x[:ns] = np.arange(ns, dtype=f32) + f32(0.999)
    y[:ns] = np.array([0.0, 0.5, 0.999, 0.25] * 3, f32)[:ns]
    if n > 12:
        x[12], y[12] = f32(10.999), f32(3.5)
    if n > 13:
        x[13], y[13] = f32(-0.5), f32(-0.999)     # truncates to (0, 0): inside
    assert (np.trunc(x) < MAP_W).all() and (np.trunc(y) < MAP_H).all()
    k["x"], k["y"] = x, y
    if with_outside:
        k["x"][n - 2] = f32(MAP_W)
        k["x"][n - 1], k["y"][n - 1] = f32(np.nan), f32(1.0)
    ku = k.copy()
    ku["x"] = k["x"] + (rng.random(n) * 7 + 1).astype(f32)
    ku["y"] = k["y"] - f32(2.0)
    return k, ku
