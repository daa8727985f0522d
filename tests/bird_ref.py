"""A plain reference of the birdview ORB stream (cv::ORB detect, cornerSubPix, compute), written from the OpenCV
definitions and not from csrc/bird.hip or oracle/cvorb_oracle.inc: whole-image numpy where the kernels work per wave,
brute force where they are clever, Python integers / int64 where the result is exact and float64 where it is not.

Exact: FAST 9/16 (arc strength by brute force over the 16 arcs), strict 8-neighbour NMS, the mask and border
predicates, the fixed-point INTER_LINEAR resize (needed for the mask pyramid), the Harris integer sums, the two patch
moments, the fixed-point 7 x 7 blur with both rounding rules, the one-level descriptor at 0 and 90 degrees.
float64: the Harris response from the exact sums, atan2 in degrees, cornerSubPix with plain bilinear sampling (no
recurrence, no 1e-4 clamp) and a per-iteration trace.  Selection is a set: the top n and every tie of the n-th."""
import functools
import math
import os
import re

import numpy as np

EDGE = 31
FAST_T = 20
HALF_PATCH = 15
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))   # Bresenham circle, radius 3
HARRIS_K = float(np.float32(0.04))
_s = np.float32(1.0) / np.float32(4 * 7 * 255.0)
HARRIS_SCALE4 = float(_s * _s * _s * _s)      # the float32 value the code multiplies by


def pattern():
    """The 256 rBRIEF pairs (x0, y0, x1, y1): data table of the repository (oracle/pattern31_data.inc)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "pattern31_data.inc")
    body = open(path).read().split("ORACLE_PATTERN31_VALUES", 1)[1]
    v = np.array([int(t) for t in re.findall(r"-?\d+", body)], np.int64)
    assert v.size == 1024
    return v.reshape(256, 4)


# ---------------------------------------------------------------- FAST, NMS, predicates
def arc_strength(img):
    """s(x, y) = max over the 16 arcs of 9 contiguous ring pixels of the arc's weakest signed contrast, brighter or
    darker: every pixel of some arc is brighter than v + t or darker than v - t exactly when s > t.  0 within 3 px
    of the image edge."""
    im = np.asarray(img).astype(np.int64)
    h, w = im.shape
    s = np.zeros((h, w), np.int64)
    c = im[3:h - 3, 3:w - 3]
    d = np.stack([im[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])   # ring - centre
    best = np.zeros_like(c)
    for k in range(16):
        arc = d[[(k + i) % 16 for i in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))   # all brighter / all darker
    s[3:h - 3, 3:w - 3] = best
    return s


def fast_scores(img, t=FAST_T):
    """cv::FAST's corner score: the largest threshold at which the pixel is still a corner, s - 1, where s > t."""
    s = arc_strength(img)
    return np.where(s > t, s - 1, 0)


def nms(score):
    """Strictly greater than all 8 neighbours."""
    h, w = score.shape
    p = np.zeros((h + 2, w + 2), score.dtype)
    p[1:-1, 1:-1] = score
    keep = score > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= score > p[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
    return keep


def in_border(x, y, w, h, edge=EDGE):
    """runByImageBorder: Rect(edge, edge, w - 2 edge, h - 2 edge).contains((x, y)); an image not larger than the
    border keeps nothing."""
    return w > 2 * edge and h > 2 * edge and edge <= x < w - edge and edge <= y < h - edge


def candidates(img, mask=None, t=FAST_T, edge=EDGE):
    """[(x, y, score)] in raster order: FAST corners that win the NMS, lie on a non-zero mask pixel and inside the
    border.  Corners outside the border are scored and take part in the NMS."""
    sc = fast_scores(img, t)
    h, w = sc.shape
    ys, xs = np.nonzero(nms(sc))
    return [(int(x), int(y), int(sc[y, x])) for x, y in zip(xs, ys)
            if (mask is None or mask[y, x] != 0) and in_border(x, y, w, h, edge)]


# ---------------------------------------------------------------- pyramid (fixed point, exact)
def cv_round(v):
    return int(np.rint(v))


def level_sizes(w, h, nlevels, scale_factor=1.2):
    sf = float(np.float32(scale_factor))
    out = []
    for l in range(nlevels):
        s = np.float32(sf ** l)
        out.append((cv_round(np.float32(w) / s), cv_round(np.float32(h) / s), float(s)))
    return out


@functools.lru_cache(maxsize=None)
def _coef(dn, sn):
    scale = 1.0 / (dn / sn)
    ofs, c0, c1 = [], [], []
    for d in range(dn):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            f, s = np.float32(0), 0
        if s >= sn - 1:
            f, s = np.float32(0), sn - 1
        ofs.append(s)
        c0.append(cv_round((np.float32(1) - f) * np.float32(2048)))
        c1.append(cv_round(f * np.float32(2048)))
    return np.array(ofs), np.array(c0, np.int64), np.array(c1, np.int64)


def resize_linear(src, dw, dh):
    """cv::resize(INTER_LINEAR) of an 8-bit image in OpenCV 3.2's fixed point: 11-bit coefficients, the horizontal
    sums kept at 11 fractional bits, the vertical pass on sums shifted right by 4 with each product shifted right by
    16, then (a + b + 2) >> 2."""
    s = np.asarray(src).astype(np.int64)
    sh, sw = s.shape
    xo, xa, xb = _coef(dw, sw)
    yo, ya, yb = _coef(dh, sh)
    x1 = np.minimum(xo + 1, sw - 1)
    y1 = np.minimum(yo + 1, sh - 1)
    hor = s[:, xo] * xa + s[:, x1] * xb
    top, bot = hor[yo] >> 4, hor[y1] >> 4
    return ((((ya[:, None] * top) >> 16) + ((yb[:, None] * bot) >> 16) + 2) >> 2).astype(np.uint8)


def pyramid(img, nlevels, is_mask=False):
    out = [np.asarray(img, np.uint8)]
    for w, h, _ in level_sizes(img.shape[1], img.shape[0], nlevels)[1:]:
        nxt = resize_linear(out[-1], w, h)
        if is_mask:
            nxt = np.where(nxt > 254, nxt, 0).astype(np.uint8)   # threshold(254, 0, THRESH_TOZERO)
        out.append(nxt)
    return out


def footprint(w, h):
    """Frame.cc:320-327: the vehicle rectangle (+15 px) that is zeroed in the mask, as (x0, y0, x1, y1), clipped."""
    p2m, length, width, b = 0.03984 * 1.7, 4.63, 1.901, 15.0
    rx, ry = int(w // 2 - width / 2 / p2m - b), int(h // 2 - length / 2 / p2m - b)
    rw, rh = int(width / p2m + 2 * b), int(length / p2m + 2 * b)
    return max(rx, 0), max(ry, 0), min(rx + rw, w), min(ry + rh, h)


def footprint_mask(mask):
    m = np.array(mask, np.uint8)
    x0, y0, x1, y1 = footprint(m.shape[1], m.shape[0])
    m[y0:y1, x0:x1] = 0
    return m


# ---------------------------------------------------------------- Harris, moments, angle
def harris_sums(img, x, y):
    """(ixx, iyy, ixy) over the 7 x 7 block around (x, y): Sobel-weighted differences, Python integers."""
    im = np.asarray(img).astype(np.int64)
    a = b = c = 0
    for j in range(y - 3, y + 4):
        for i in range(x - 3, x + 4):
            ix = 2 * (im[j, i + 1] - im[j, i - 1]) + (im[j - 1, i + 1] - im[j - 1, i - 1]) + (im[j + 1, i + 1] - im[j + 1, i - 1])
            iy = 2 * (im[j + 1, i] - im[j - 1, i]) + (im[j + 1, i - 1] - im[j - 1, i - 1]) + (im[j + 1, i + 1] - im[j - 1, i + 1])
            a += int(ix * ix)
            b += int(iy * iy)
            c += int(ix * iy)
    return a, b, c


def harris_response(sums):
    a, b, c = sums
    return (a * b - c * c - HARRIS_K * (a + b) * (a + b)) * HARRIS_SCALE4


def harris_bound(sums):
    """8 float32 roundings on magnitudes up to (ixx + iyy)^2, scaled: 2^-20 (ixx + iyy)^2 scale^4."""
    return 2.0 ** -20 * (sums[0] + sums[1]) ** 2 * HARRIS_SCALE4


def patch_halfwidths():
    """orb.cpp u_max: the half-width of each row of the radius-15 patch, made symmetric about the diagonal."""
    hp = HALF_PATCH
    vmax, vmin = int(math.floor(hp * math.sqrt(2.0) / 2 + 1)), int(math.ceil(hp * math.sqrt(2.0) / 2))
    u = [0] * (hp + 2)
    for v in range(vmax + 1):
        u[v] = cv_round(math.sqrt(hp * hp - v * v))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u[:hp + 1]


def moments(img, x, y):
    """(m10, m01) of the circular patch around (x, y)."""
    im = np.asarray(img).astype(np.int64)
    um = patch_halfwidths()
    m10 = m01 = 0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        for u in range(-um[abs(v)], um[abs(v)] + 1):
            m10 += u * int(im[y + v, x + u])
            m01 += v * int(im[y + v, x + u])
    return m10, m01


def angle_deg(m10, m01):
    a = math.degrees(math.atan2(m01, m10))
    return a + 360.0 if a < 0 else a


def fast_atan2_diagonal():
    """cv::fastAtan2 where |y| == |x| != 0: c = 1, so the result is the float32 Horner sum of the four coefficients."""
    f = np.float32
    sc = f(180.0 / math.pi)
    p1, p3, p5, p7 = (f(0.9997878412794807) * sc, f(-0.3258083974640975) * sc, f(0.1555786518463281) * sc,
                      f(-0.04432655554792128) * sc)
    return f(f(f(f(f(f(p7 + p5)) + p3)) + p1))


def fast_atan2_small(m10, m01):
    """cv::fastAtan2 for |m01| <= m10 in float32, step by step (used for the near-360 plant)."""
    f = np.float32
    sc = f(180.0 / math.pi)
    p1, p3, p5, p7 = (f(0.9997878412794807) * sc, f(-0.3258083974640975) * sc, f(0.1555786518463281) * sc,
                      f(-0.04432655554792128) * sc)
    c = f(abs(m01)) / f(f(m10) + f(2.220446049250313e-16))
    c2 = f(c * c)
    a = f(f(f(f(f(f(f(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c)
    return f(f(360.0) - a) if m01 < 0 else a


# ---------------------------------------------------------------- selection
def retain_best(items, n):
    """KeyPointsFilter::retainBest as a set: items is [(key, response)]; the n largest and every tie of the n-th."""
    if n < 0 or len(items) <= n:
        return {k for k, _ in items}
    if n == 0:
        return set()
    cut = sorted((r for _, r in items), reverse=True)[n - 1]
    return {k for k, r in items if r >= cut}


def detect_set(img, mask, nfeat_per_level, nlevels=1):
    """{(level, x, y)} that cv::ORB::detect returns (level coordinates), with the per-level candidate lists."""
    lv = pyramid(img, nlevels)
    mk = pyramid(mask, nlevels, True) if mask is not None else [None] * nlevels
    out, cands = set(), []
    for l in range(nlevels):
        c = candidates(lv[l], mk[l])
        cands.append(c)
        first = retain_best([((x, y), s) for x, y, s in c], 2 * nfeat_per_level[l])
        resp = [(k, harris_response(harris_sums(lv[l], *k))) for k in sorted(first)]
        out |= {(l, x, y) for x, y in retain_best(resp, nfeat_per_level[l])}
    return out, cands, lv


# ---------------------------------------------------------------- blur, descriptor
def gauss_q8():
    x = np.arange(7) - 3.0
    cf = np.exp(-0.5 / 4.0 * x * x).astype(np.float32)
    k = (cf.astype(np.float64) * (1.0 / cf.astype(np.float64).sum())).astype(np.float32)
    return np.rint(k * np.float32(256)).astype(np.int64)


def blur_sums(img):
    """The 16-fractional-bit sums of GaussianBlur(7 x 7, sigma 2, BORDER_REFLECT_101), int64."""
    k = gauss_q8()
    p = np.pad(np.asarray(img).astype(np.int64), 3, mode="reflect")
    h, w = np.asarray(img).shape
    s = np.zeros((h, w), np.int64)
    for i in range(7):
        for j in range(7):
            s += k[i] * k[j] * p[i:i + h, j:j + w]
    return s


def blur(img, rule="opencv"):
    """rule "opencv": half-to-even on columns below w & ~3 (the SSE2 body), half-up on the rest; "half_up" /
    "half_even": one rule on every column (used to show that a plant depends on the rule)."""
    s = blur_sums(img)
    w = s.shape[1]
    q, rem = s >> 16, s & 0xFFFF
    even = np.where(rem > 32768, q + 1, np.where(rem < 32768, q, q + (q & 1)))
    up = (s + 32768) >> 16
    if rule == "opencv":
        v = np.where(np.arange(w)[None, :] < (w & ~3), even, up)
    else:
        v = up if rule == "half_up" else even
    return np.clip(v, 0, 255).astype(np.uint8)


def sample_offsets(angle, strict=True):
    """The 512 rounded pattern offsets at `angle` degrees (float64 rotation; exact integers at 0, within 1e-5 of
    integers at 90, so the rounding is never at a half).  strict=False: any angle, for counting samples only."""
    a = float(np.float32(angle) * np.float32(math.pi / 180.0))
    ca, sa = math.cos(a), math.sin(a)
    p = pattern().reshape(512, 2).astype(np.float64)
    x = p[:, 0] * ca - p[:, 1] * sa
    y = p[:, 0] * sa + p[:, 1] * ca
    assert not strict or max(np.abs(x - np.rint(x)).max(), np.abs(y - np.rint(y)).max()) < 1e-3, "only for quarter turns"
    return np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)


def descriptor(blurred, cx, cy, angle):
    """The 32 bytes of a level-0 keypoint whose rounded position is (cx, cy): bit p = blurred[first] < blurred[second]."""
    ox, oy = sample_offsets(angle)
    v = blurred[cy + oy, cx + ox].astype(np.int64).reshape(256, 2)
    bits = (v[:, 0] < v[:, 1]).astype(np.uint8)
    return np.packbits(bits, bitorder="little"), v


# ---------------------------------------------------------------- cornerSubPix, float64
SINGULAR, LEFT_IMAGE, EPS, MAX_ITER = "singular", "left_image", "eps", "max_iter"


def _bilinear(im, x, y):
    h, w = im.shape
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xi = lambda v: np.clip(v.astype(np.int64), 0, w - 1)
    yi = lambda v: np.clip(v.astype(np.int64), 0, h - 1)
    return (im[yi(y0), xi(x0)] * (1 - fx) * (1 - fy) + im[yi(y0), xi(x0 + 1)] * fx * (1 - fy) +
            im[yi(y0 + 1), xi(x0)] * (1 - fx) * fy + im[yi(y0 + 1), xi(x0 + 1)] * fx * fy)


def corner_subpix(img, pt, win=5, max_iter=40, eps=0.001):
    """cv::cornerSubPix for one point in float64: replicate-border bilinear samples on the 13 x 13 grid around the
    current estimate, central differences, the Gaussian window exp(-(i/win)^2) exp(-(j/win)^2), the 2 x 2 normal
    equations.  Returns ((x, y), trace, reset); trace holds one dict per iteration: the position it started from, its
    offset from the start point, the patch's first pixel (ipx, ipy), whether the 13 x 13 patch lay inside the image,
    the determinant, and `exit` on the
    last one."""
    im = np.asarray(img).astype(np.float64)
    h, w = im.shape
    g = np.arange(-win, win + 1, dtype=np.float64)
    wgt = np.exp(-(g / win) ** 2)[:, None] * np.exp(-(g / win) ** 2)[None, :]
    px, py = np.meshgrid(g, g)
    gp = np.arange(-win - 1, win + 2, dtype=np.float64)
    sx, sy = float(np.float32(pt[0])), float(np.float32(pt[1]))
    cx, cy, trace, why = sx, sy, [], MAX_ITER
    for it in range(max_iter):
        X, Y = np.meshgrid(cx + gp, cy + gp)
        patch = _bilinear(im, X, Y)
        ipx, ipy = math.floor(cx - win - 1), math.floor(cy - win - 1)
        rec = dict(pos=(cx, cy), off=max(abs(cx - sx), abs(cy - sy)), ipx=ipx, ipy=ipy,
                   inside=0 <= ipx and ipx + 2 * win + 3 < w and 0 <= ipy and ipy + 2 * win + 3 < h,
                   integer_x=cx - win - 1 == ipx)
        trace.append(rec)
        gx = patch[1:-1, 2:] - patch[1:-1, :-2]
        gy = patch[2:, 1:-1] - patch[:-2, 1:-1]
        a, b, c = (gx * gx * wgt).sum(), (gx * gy * wgt).sum(), (gy * gy * wgt).sum()
        b1 = ((gx * gx * px + gx * gy * py) * wgt).sum()
        b2 = ((gx * gy * px + gy * gy * py) * wgt).sum()
        det = a * c - b * b
        rec["det"] = det
        if abs(det) <= np.finfo(np.float64).eps ** 2:
            why = SINGULAR
            break
        nx, ny = cx + (c * b1 - b * b2) / det, cy + (a * b2 - b * b1) / det
        err = (nx - cx) ** 2 + (ny - cy) ** 2
        cx, cy = nx, ny
        if cx < 0 or cx >= w or cy < 0 or cy >= h:
            why = LEFT_IMAGE
            break
        if err <= eps * eps:
            why = EPS
            break
    trace[-1]["exit"] = why
    reset = abs(cx - sx) > win or abs(cy - sy) > win
    return ((sx, sy) if reset else (cx, cy)), trace, reset


def features_per_level(nfeatures, nlevels, scale_factor=1.2):
    """orb.cpp: a geometric series over the levels in float32, rounded; the last level takes the remainder."""
    f = np.float32
    factor = f(1.0 / float(f(scale_factor)))
    nd = f(nfeatures) * (f(1) - factor) / (f(1) - f(float(factor) ** nlevels))
    out = []
    for _ in range(nlevels - 1):
        out.append(cv_round(nd))
        nd = f(nd * factor)
    return out + [max(nfeatures - sum(out), 0)]
