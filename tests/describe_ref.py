"""Test-side restatement of what k_describe fuses (csrc/extract_kernels.hip): IC_Angle (ORBextractor.cc:77-104), the
pinned GaussianBlur 7x7 sigma 2 (:1085-1086; OpenCV 3.2's 8U path: exact integer row pass, column pass rounded
half-to-even where SymmColumnVec_32s8u runs, x < (w & ~3), and half-up in the scalar tail) and computeOrbDescriptor
(:108-147) with the reference build's contracted sample offsets.  Plain NumPy: integer moments, integer blur sums
with the rounding spelled out, cv::fastAtan2 in float32 operation by operation, an exact float32 fma, and glibc's
sinf / cosf through the oracle's restatement (oracle.sincosf; the one piece not restated twice).

describe() returns one Trace per keypoint: the moments, the angle, a and b, and per pattern point the sample offset,
the blur sum S at that pixel, whether the pixel lies in the scalar tail, and the rounded (unsaturated) value; per
test the bit.  Every rule the kernel's hand-made tricks depend on is a field of Rules, so a test can mutate one rule
and see which planted cases notice (tests/test_describe_cases.py)."""
import collections

import numpy as np

f32 = np.float32
HALF_PATCH = 15
PATCH_SIZE = 31
FACTOR_PI = f32(np.pi / float(f32(180.0)))                    # (float)(CV_PI / 180.f), ORBextractor.cc:107

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

# One rule per decision family; the defaults are the pinned reference build.
#   blur      "pinned" (half-even below xsimd, half-up from it), "halfup" (ORB_VARIANT_BLUR_HALFUP), "halfeven"
#             (everywhere), "noparity" (pinned, but a body tie rounds down: the (S >> 16) & 1 term dropped)
#   tail      added to xsimd = w & ~3 (the tail boundary off by one)
#   fma       sample offsets contracted (False: ORB_VARIANT_NO_FMA)
#   trig      "glibc" or "cr" (correctly rounded, the oracle's TRIG_CR)
#   cvround   "even" or "away"
#   cmp       "lt" or "le"
#   sat       "both" (the reference compares uchar pixels; the kernel clamps the right side only, which is the same
#             predicate, see saturate_forms), "none", "left"
#   border    "reflect" (REFLECT_101) or "replicate"
#   umax_row, umax_delta   umax[row] += delta in IC_Angle
Rules = collections.namedtuple("Rules", "blur tail fma trig cvround cmp sat border umax_row umax_delta")
PINNED = Rules("pinned", 0, True, "glibc", "even", "lt", "both", "reflect", 0, 0)

Trace = collections.namedtuple("Trace", "level x y m01 m10 angle a b ox oy S tail val bits desc")


def gauss_kernel():
    """getGaussianKernel(7, 2, CV_32F) scaled by 256 and rounded (FilterEngine's fixed-point taps)."""
    x = np.arange(7) - 3.0
    cf = np.exp(-0.125 * x * x).astype(f32)
    s = 1.0 / cf.astype(np.float64).sum()
    cf = (cf.astype(np.float64) * s).astype(f32)
    return np.rint(cf * f32(256.0)).astype(np.int64)


K = gauss_kernel()
assert K.tolist() == [18, 34, 49, 55, 49, 34, 18] and int(K.sum()) == 257


def umax_table():
    """ORBextractor.cc:452-469."""
    hp = HALF_PATCH
    half = f32(f32(hp) * np.sqrt(f32(2.0)) / f32(2.0))
    vmax, vmin = int(np.floor(half + f32(1.0))), int(np.ceil(half))
    um = [0] * (hp + 1)
    for v in range(vmax + 1):
        um[v] = int(np.rint(np.sqrt(float(hp * hp - v * v))))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while um[v0] == um[v0 + 1]:
            v0 += 1
        um[v] = v0
        v0 += 1
    return um


UMAX = umax_table()


def fast_atan2(y, x):
    """cv::fastAtan2 (OpenCV 3.2 mathfuncs_core), float32 operation by operation, on arrays."""
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    s = f32(180.0 / np.pi)
    p1, p3 = f32(0.9997878412794807) * s, f32(-0.3258083974640975) * s
    p5, p7 = f32(0.1555786518463281) * s, f32(-0.04432655554792128) * s
    eps = f32(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    ge = ax >= ay
    num, den = np.where(ge, ay, ax), np.where(ge, ax, ay) + eps
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (num / den).astype(f32)
    c2 = (c * c).astype(f32)
    poly = ((((p7 * c2).astype(f32) + p5).astype(f32) * c2).astype(f32) + p3).astype(f32)
    poly = ((((poly * c2).astype(f32) + p1).astype(f32)) * c).astype(f32)
    a = np.where(ge, poly, (f32(90.0) - poly).astype(f32)).astype(f32)
    a = np.where(x < 0, (f32(180.0) - a).astype(f32), a)
    a = np.where(y < 0, (f32(360.0) - a).astype(f32), a)
    return a.astype(f32)


def fma32(a, b, c):
    """float32 fma on arrays: a * b is exact in float64, the sum is rounded to odd there (the float64 neighbour of
    the exact sum with an odd mantissa), and 53 >= 24 + 2 bits make the final rounding to float32 the single one."""
    a, b, c = (np.asarray(v, f32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                           # TwoSum: p + c == s + err exactly
    even = (s.view(np.int64) & 1) == 0
    other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, other, s).astype(f32)


def sincos(angle_rad, trig):
    import oracle
    x = np.atleast_1d(np.asarray(angle_rad, f32))
    if trig == "cr":
        return np.sin(x.astype(np.float64)).astype(f32), np.cos(x.astype(np.float64)).astype(f32)
    return oracle.sincosf(x)


def pattern_points():
    """(512, 2) float32: bit_pattern_31_ as (x, y); test t compares points 2t and 2t + 1."""
    import oracle
    return oracle.pattern().reshape(512, 2).astype(f32)


def cv_round(v, mode):
    v = np.asarray(v, f32).astype(np.float64)
    if mode == "away":
        return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)
    return np.rint(v).astype(np.int64)


def sample_coords(angle, rules=PINNED, pat=None):
    """Per pattern point the float sample offset (fx, fy) before cvRound, :113-120, for an (n,) array of angles in
    degrees: (n, 512) arrays, and (a, b)."""
    pat = pattern_points() if pat is None else pat
    ang = np.atleast_1d(np.asarray(angle, f32))
    b, a = sincos((ang * FACTOR_PI).astype(f32), rules.trig)
    a2, b2 = a[:, None], b[:, None]
    px, py = pat[None, :, 0], pat[None, :, 1]
    if rules.fma:
        fy = fma32(px, b2, (py * a2).astype(f32))
        fx = fma32(px, a2, -(py * b2).astype(f32))
    else:
        fy = ((px * b2).astype(f32) + (py * a2).astype(f32)).astype(f32)
        fx = ((px * a2).astype(f32) - (py * b2).astype(f32)).astype(f32)
    return fx, fy, a, b


def sample_offsets(angle, rules=PINNED, pat=None):
    """Per pattern point the integer sample offset (ox, oy) from the keypoint; `angle` in degrees, a scalar or an
    (n,) array (then (n, 512) results).  Also returns (a, b)."""
    fx, fy, a, b = sample_coords(angle, rules, pat)
    ox, oy = cv_round(fx, rules.cvround), cv_round(fy, rules.cvround)
    if np.ndim(angle) == 0:
        return ox[0], oy[0], a[0], b[0]
    return ox, oy, a, b


def moments(img, x, y, rules=PINNED):
    """(m01, m10) of IC_Angle: integer sums over the circular patch |u| <= umax[|v|]."""
    um = list(UMAX)
    um[rules.umax_row] += rules.umax_delta
    m01 = m10 = 0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        d = um[abs(v)]
        row = img[y + v, x - d:x + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m01, m10


def blur_sums(img, rules=PINNED):
    """S[y, x] = sum_ij K[i] K[j] p(y + i - 3, x + j - 3) with the border rule: the column pass's integer sum before
    its rounding (blurred = round(S / 65536))."""
    p = np.pad(img.astype(np.int64), 3, mode="reflect" if rules.border == "reflect" else "edge")
    h, w = img.shape
    R = sum(int(K[t]) * p[:, t:t + w] for t in range(7))
    return sum(int(K[t]) * R[t:t + h, :] for t in range(7))


def round_blur(S, x, w, rules=PINNED):
    """(rounded value before saturate_cast, in the scalar tail) of sums S at columns x of a level w wide."""
    S, x = np.asarray(S, np.int64), np.asarray(x, np.int64)
    q, rem = S >> 16, S & 0xFFFF
    up = (S + 32768) >> 16
    tie_up = (q & 1) if rules.blur != "noparity" else 0
    even = np.where(rem > 32768, q + 1, np.where(rem < 32768, q, q + tie_up))
    xsimd = {"halfup": 0, "halfeven": w + 64}.get(rules.blur, (w & ~3) + rules.tail)
    tail = x >= xsimd
    return np.where(tail, up, even), tail


def blur(img, rules=PINNED):
    """The blurred level as the reference stores it (uchar)."""
    h, w = img.shape
    v, _ = round_blur(blur_sums(img, rules), np.arange(w)[None, :], w, rules)
    return np.clip(v, 0, 255).astype(np.uint8)


def saturate_forms(v0, v1):
    """The test's predicate as the reference evaluates it (both pixels uchar) and as k_describe does (the right side
    clamped only): equal for all values a 7x7 blur of bytes can give (0..257)."""
    return min(v0, 255) < min(v1, 255), v0 < min(v1, 255)


def compare(v0, v1, rules=PINNED):
    v0, v1 = np.asarray(v0, np.int64), np.asarray(v1, np.int64)
    if rules.sat == "both":
        v0, v1 = np.minimum(v0, 255), np.minimum(v1, 255)
    elif rules.sat == "left":
        v0 = np.minimum(v0, 255)
    return v0 <= v1 if rules.cmp == "le" else v0 < v1


def describe(img, pts, level=0, rules=PINNED, pat=None):
    """One Trace per keypoint (x, y) of the level image `img`."""
    pat = pattern_points() if pat is None else pat
    h, w = img.shape
    S_img = blur_sums(img, rules)
    out = []
    for (x, y) in pts:
        x, y = int(x), int(y)
        m01, m10 = moments(img, x, y, rules)
        angle = f32(fast_atan2(f32(m01), f32(m10)))
        ox, oy, a, b = sample_offsets(angle, rules, pat)
        S = S_img[y + oy, x + ox]
        val, tail = round_blur(S, x + ox, w, rules)
        bits = compare(val[0::2], val[1::2], rules).astype(np.uint8)
        out.append(Trace(level, x, y, m01, m10, angle, a, b, ox, oy, S, tail, val, bits,
                         np.packbits(bits, bitorder="little")))
    return out


def scale_factors(scale, nlevels):
    """mvScaleFactor (:419-426): float products of a double scaleFactor."""
    s = [f32(1.0)]
    for _ in range(1, nlevels):
        s.append(f32(float(s[-1]) * float(f32(scale))))
    return s


def extract(levels, level_kps, scale, rules=PINNED):
    """Keypoints (KP_DTYPE), descriptors and traces of a frame, from its level images and each level's retained
    keypoints as (x, y, response) rows in the octree's order (:1058-1103): detection is not restated here."""
    sf = scale_factors(scale, len(levels))
    pat = pattern_points()
    kps, traces = [], []
    for l, (img, lk) in enumerate(zip(levels, level_kps)):
        tr = describe(img, [(r[0], r[1]) for r in lk], l, rules, pat)
        for r, t in zip(lk, tr):
            fx, fy = f32(t.x), f32(t.y)
            if l != 0:
                fx, fy = fx * sf[l], fy * sf[l]
            kps.append((fx, fy, f32(int(PATCH_SIZE * sf[l])), t.angle, f32(r[2]), l, -1))
        traces += tr
    k = np.array(kps, KP_DTYPE) if kps else np.zeros(0, KP_DTYPE)
    d = np.stack([t.desc for t in traces]) if traces else np.zeros((0, 32), np.uint8)
    return k, d, traces
