"""Named, deterministic inputs that force the decisions of the birdview ORB stream (csrc/bird.hip: cv::ORB detect,
cornerSubPix, compute).  Pure numpy.  tests/test_bird_cases.py checks on the CPU that tests/bird_ref.py realises every
plant and agrees with the oracle; tests/test_gpu_bird_cases.py requires the GPU to equal the oracle byte for byte and
to show every plant.

One-level cases are 192 x 160 (candidate columns 31..160 span the lane chunks 31..94 | 95..158 | 159..160 of
k_bird_cands) with BirdORB(nfeatures, 1.2, 1, 31, 20); the mask-pyramid and high-octave cases are 320 x 240 with 8
levels; the one-level blur case is 190 wide (tail columns 188, 189).  The building block of the detect cases is a STAMP: one
pixel of value v on a flat background b.  Its ring is the background, so its arc strength is |v - b| and its FAST
score |v - b| - 1; no other pixel near it is a corner (a ring through the stamp holds one differing pixel), so stamps
12 px apart do not see each other in FAST, NMS or Harris.  Pixels that only shift a moment differ from the background
by at most the threshold (20) and are never corners.

A case is built once and never modified.  A plant is (item, what, where, expect):
  cand     where (level, x, y); expect (present, raw): in the candidate list or not, and the pixel's FAST score
  count    where tuple of (level, x, y); expect how many of them detect() returns
  angle    where (level, x, y); expect ("exact", float32) or ("near", m10, m01)
  harris   where (level, x, y); expect "above_2p24" or "negative"
  extract  where (x, y); expect a keypoint within 1.5 px in extract()'s output
  subpix   where index into case.pts; expect a dict (see subpix())
  desc     where index into case.kps; expect a dict (see the compute cases)
  blur     where (x, y) or (x, y, level); expect (quotient, value)"""
import collections
import functools
import math

import numpy as np

import bird_ref as ref

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
W1, H1 = 192, 160
W8, H8 = 320, 240

Case = collections.namedtuple("Case", "name kind img mask nfeat nlevels plants pts kps")
Plant = collections.namedtuple("Plant", "item what where expect")

ITEMS = (
    # 1.1 detect
    "fast_arc_9_kept", "fast_arc_8_dropped", "fast_ring_at_threshold", "fast_score_255_minus_1",
    "nms_equal_neighbours_both_dropped", "nms_one_higher_wins", "nms_across_lane_chunk", "border_first_kept",
    "border_outside_dropped", "border_neighbour_suppresses", "mask_value_1_keeps_level0", "mask_254_drops_level1",
    "footprint_edge",
    # 1.2 Harris and selection
    "harris_sum_above_2p24", "harris_negative", "retain_ties_all_kept", "retain_cut_with_margin",
    # 1.3 orientation
    "angle_symmetric_zero", "angle_axes", "angle_diagonals", "angle_near_360",
    # 1.4 cornerSubPix
    "subpix_flat_unchanged", "subpix_ideal_corner", "subpix_reset_over_5px", "subpix_leaves_image",
    "subpix_border_replicate", "subpix_uncached_inside", "subpix_leaves_cache", "subpix_40_iterations",
    "subpix_eps_exit_first_iteration",
    # 1.5 descriptors
    "desc_flat_all_zero", "desc_angle_0", "desc_angle_90", "desc_pair_differs_by_one", "desc_outside_roi",
    "desc_culled_by_border",
    # 1.6 blur
    "blur_exact_half",
)

# cornerSubPix on the starts around the two checker corners (subpix_ideal_corner, subpix_uncached_inside), measured
# on the CPU with
#   python -m pytest tests/test_bird_cases.py -k subpix_ideal -s
# (it prints both maxima): the oracle's largest distance (max norm, px) to bird_ref's float64 result and to the
# analytic corner.  The GPU test asserts twice these; the GPU must equal the oracle's bytes anyway.
SUBPIX_ORACLE_TO_REF = 4.1e-6          # measured 4.07e-06
SUBPIX_ORACLE_TO_ANALYTIC = 6.96e-2    # measured 0.0695 (the box-filtered, 8-bit corner is not the ideal one)


def _flat(v, w=W1, h=H1):
    return np.full((h, w), v, np.uint8)


def _done(name, kind, img, plants, mask=None, nfeat=500, nlevels=1, pts=None, kps=None):
    arrs = [img] + [a for a in (mask, pts, kps) if a is not None]
    for a in arrs:
        a.setflags(write=False)
    return Case(name, kind, img, mask, nfeat, nlevels, tuple(plants), pts, kps)


def _cand(item, x, y, present, raw, level=0):
    return Plant(item, "cand", (level, x, y), (present, raw))


# ------------------------------------------------------------------------------------------ 1.1 detect
def _fast():
    img, pl = _flat(100), []
    # a 9-arc of ring pixels 21 above / below the centre makes it a corner of score 20; an 8-arc does not
    for n, (sign, start, length) in enumerate(((1, 2, 9), (1, 5, 8), (-1, 7, 9), (-1, 12, 8))):
        x, y = 48 + 24 * n, 48
        for i in range(length):
            dx, dy = ref.RING[(start + i) % 16]
            img[y + dy, x + dx] = 100 + 21 * sign
        pl.append(_cand("fast_arc_9_kept" if length == 9 else "fast_arc_8_dropped", x, y, length == 9,
                        20 if length == 9 else 0))
    # the whole ring exactly t from the centre: no corner; t + 1: a corner of score t
    for n, v in enumerate((120, 121, 80, 79)):
        x, y = 48 + 24 * n, 80
        img[y, x] = v
        pl.append(_cand("fast_ring_at_threshold", x, y, abs(v - 100) == 21, 20 if abs(v - 100) == 21 else 0))
    return _done("fast", "detect", img, pl)


def _fast255():
    img = _flat(255)
    img[80, 96] = 0
    return _done("fast255", "detect", img, [_cand("fast_score_255_minus_1", 96, 80, True, 254)])


def _nms_image():
    img, pl = _flat(100), []

    def pair(item, a, va, b, vb):
        img[a[1], a[0]], img[b[1], b[0]] = va, vb
        pl.append(_cand(item, *a, va > vb, va - 101))
        pl.append(_cand(item, *b, vb > va, vb - 101))

    for a, b in (((50, 40), (51, 40)), ((70, 40), (70, 41)), ((90, 40), (91, 41)), ((111, 40), (110, 41))):
        pair("nms_equal_neighbours_both_dropped", a, 150, b, 150)
    pair("nms_one_higher_wins", (130, 40), 150, (131, 40), 160)
    pair("nms_one_higher_wins", (145, 41), 160, (144, 40), 150)
    for x in (94, 158):          # the last lane of one 64-column chunk and the first of the next
        pair("nms_across_lane_chunk", (x, 60), 150, (x + 1, 60), 150)
        pair("nms_across_lane_chunk", (x, 72), 150, (x + 1, 72), 160)
        pair("nms_across_lane_chunk", (x, 84), 160, (x + 1, 84), 150)
    for x, y, inside in ((31, 100, True), (W1 - 32, 100, True), (30, 112, False), (W1 - 31, 112, False),
                         (60, 31, True), (60, H1 - 32, True), (76, 30, False), (76, H1 - 31, False),
                         (31, 31, True), (W1 - 32, H1 - 32, True)):
        img[y, x] = 150
        pl.append(_cand("border_first_kept" if inside else "border_outside_dropped", x, y, inside, 49))
    for a, b in (((30, 124), (31, 124)), ((100, 30), (100, 31)), ((W1 - 31, 66), (W1 - 32, 67)),
                 ((120, H1 - 31), (120, H1 - 32))):   # the stronger corner outside the border still suppresses
        img[a[1], a[0]], img[b[1], b[0]] = 160, 150
        pl.append(_cand("border_neighbour_suppresses", *a, False, 59))
        pl.append(_cand("border_neighbour_suppresses", *b, False, 49))
    return img, pl


def _nms():
    img, pl = _nms_image()
    return _done("nms_border", "detect", img, pl)


def _mask0():
    img, _ = _nms_image()
    mask = _flat(255)
    mask[100, 31] = 1          # any non-zero value keeps a level-0 candidate
    mask[31, 60] = 128
    mask[100, W1 - 32] = 0
    mask[40:42, 130:132] = 0   # the winner of a pair is masked: the loser stays suppressed
    pl = [_cand("mask_value_1_keeps_level0", 31, 100, True, 49), _cand("mask_value_1_keeps_level0", 60, 31, True, 49),
          _cand("mask_value_1_keeps_level0", W1 - 32, 100, False, 49),
          _cand("mask_value_1_keeps_level0", 131, 40, False, 59), _cand("mask_value_1_keeps_level0", 130, 40, False, 49)]
    return _done("mask0", "detect", img, pl, mask=mask)


def _mask_pyr():
    """Two blobs; at level 1 each gives a candidate.  One level-0 mask pixel under the first is lowered until the
    resized mask there is exactly 254 (thresholded to 0: dropped); one under the second is lowered by so little that
    the resized mask stays 255 (kept).  Both stay non-zero at level 0."""
    img = _flat(0, W8, H8)
    for cx, cy in ((100, 100), (221, 131)):
        img[cy - 1:cy + 2, cx - 1:cx + 2] = 128
        img[cy, cx] = 255
    (w1, h1, s1) = ref.level_sizes(W8, H8, 2)[1]
    lv1 = ref.resize_linear(img, w1, h1)
    c1 = ref.candidates(lv1)
    near = lambda cx, cy: [c for c in c1 if abs(c[0] - cx / s1) < 3 and abs(c[1] - cy / s1) < 3]
    (P,), (Q,) = near(100, 100), near(221, 131)
    mask = _flat(255, W8, H8)

    def lower(c, want):
        sx, sy = int((c[0] + 0.5) * W8 / w1 - 0.5), int((c[1] + 0.5) * H8 / h1 - 0.5)
        for yy in (sy, sy + 1):
            for xx in (sx, sx + 1):
                for v in range(254, 0, -1):
                    m = mask.copy()
                    m[yy, xx] = v
                    r = ref.resize_linear(m, w1, h1)
                    if r[c[1], c[0]] == want and (want == 254 or v < 255):
                        mask[yy, xx] = v
                        return
                    if r[c[1], c[0]] < want:
                        break
        raise AssertionError("no mask value gives %d at %r" % (want, c))

    lower(P, 254)
    lower(Q, 255)
    pl = [_cand("mask_254_drops_level1", P[0], P[1], False, P[2], 1), _cand("mask_254_drops_level1", Q[0], Q[1], True, Q[2], 1)]
    return _done("mask_pyr", "detect", img, pl, mask=mask, nfeat=2000, nlevels=8)


def _footprint():
    """Through extract only: the footprint rectangle of a 192 x 160 mask is [66, 124) x [30, 128)."""
    assert ref.footprint(W1, H1) == (66, 30, 124, 128)
    img, pl = _flat(100), []
    for x, y, kept in ((65, 50, True), (66, 62, False), (123, 74, False), (124, 86, True), (90, 127, False),
                       (104, 128, True)):
        img[y, x] = 200
        pl.append(Plant("footprint_edge", "extract", (x, y), kept))
    return _done("footprint", "detect", img, pl, mask=_flat(255))


# ------------------------------------------------------------------------------------------ 1.2 Harris, selection
def _negative_block(img, x, ys):
    """A stamp between two full-height lines 4 px to either side: the lines are outside its ring and its NMS
    neighbourhood but inside its Harris block, whose response they make that of an edge (negative).  A straight line
    has no corner on it, and its ends lie on the image border."""
    img[:, x - 4] = 255
    img[:, x + 4] = 255
    for y in ys:
        img[y, x] = 100


def _harris():
    img, pl = _flat(0), []
    _negative_block(img, 64, (60,))
    pl.append(Plant("harris_negative", "harris", (0, 64, 60), "negative"))
    # vertical stripes of period 4 (|Ix| = 4 * 215 on every pixel), the centre darker than every stripe and four ring
    # pixels raised so that 13 contiguous ring pixels are bright
    x, y = 128, 80
    for dx in range(-6, 7):
        img[y - 6:y + 7, x + dx] = 255 if (dx % 4) in (2, 3) else 40
    for dx, dy in ((0, 3), (1, 3), (0, -3), (1, -3)):
        img[y + dy, x + dx] = 255
    img[y, x] = 0
    pl.append(Plant("harris_sum_above_2p24", "harris", (0, x, y), "above_2p24"))
    pl.append(_cand("harris_sum_above_2p24", x, y, True, 254))
    return _done("harris", "detect", img, pl)


SEL_A = ((50, 50), (50, 100))
SEL_B = tuple((80 + 16 * i, 50 + 20 * (i % 3)) for i in range(6))
SEL_C = ((60, 120), (100, 120), (140, 120))


def _sel(nfeat):
    """2 stamps of score 119, 6 identical of score 79, 3 identical of score 50.  nfeat 3: the FAST cut (6) falls
    inside the six, all six stay and the three go; nfeat 5: the FAST cut (10) falls inside the three, the Harris cut
    (5) inside the six.  Either way detect returns 8 keypoints, more than nfeatures."""
    img = _flat(100)
    for pts, v in ((SEL_A, 220), (SEL_B, 180), (SEL_C, 151)):
        for x, y in pts:
            img[y, x] = v
    lv = lambda pts: tuple((0, x, y) for x, y in pts)
    pl = [Plant("retain_ties_all_kept", "count", lv(SEL_B), 6), Plant("retain_ties_all_kept", "count", lv(SEL_A), 2),
          Plant("retain_ties_all_kept", "count", lv(SEL_C), 0)]
    return _done("retain_ties_nfeat%d" % nfeat, "detect", img, pl, nfeat=nfeat)


MARGIN_STRONG = ((120, 50), (120, 70), (120, 90))
MARGIN_WEAK = ((64, 50), (64, 70), (64, 90))


def _margin():
    """Three stamps of positive response and three edge-like ones of negative response; nfeatures 3 keeps exactly
    the first group (the FAST cut, 6 of 6, removes nothing)."""
    img = _flat(0)
    _negative_block(img, 64, [y for _, y in MARGIN_WEAK])
    for x, y in MARGIN_STRONG:
        img[y, x] = 200
    lv = lambda pts: tuple((0, x, y) for x, y in pts)
    pl = [Plant("retain_cut_with_margin", "count", lv(MARGIN_STRONG), 3),
          Plant("retain_cut_with_margin", "count", lv(MARGIN_WEAK), 0)]
    pl += [Plant("harris_negative", "harris", (0, x, y), "negative") for x, y in MARGIN_WEAK]
    return _done("retain_margin", "detect", img, pl, nfeat=3)


# ------------------------------------------------------------------------------------------ 1.3 orientation
def _angles():
    """One stamp per 34-pixel cell; pixels of value 20 (never corners) inside its radius-15 patch set the moments."""
    img, pl = _flat(0), []
    f = np.float32
    D = ref.fast_atan2_diagonal()
    cells = [(46 + 34 * i, 46 + 34 * j) for j in range(3) for i in range(4)]
    spec = [("angle_symmetric_zero", [], f(0)),
            ("angle_symmetric_zero", [(6, 6), (-6, -6), (9, -2), (-9, 2)], f(0)),      # point-symmetric: both moments 0
            ("angle_axes", [(10, 0)], f(0)), ("angle_axes", [(0, 10)], f(90)), ("angle_axes", [(-10, 0)], f(180)),
            ("angle_axes", [(0, -10)], f(270)),
            ("angle_diagonals", [(7, 7)], D), ("angle_diagonals", [(-7, 7)], f(180) - D),
            ("angle_diagonals", [(-7, -7)], f(360) - (f(180) - D)), ("angle_diagonals", [(7, -7)], f(360) - D)]
    for (x, y), (item, pix, want) in zip(cells, spec):
        img[y, x] = 100
        for dx, dy in pix:
            img[y + dy, x + dx] = 20
        pl.append(Plant(item, "angle", (0, x, y), ("exact", f(want))))
    x, y = cells[10]
    img[y, x] = 100
    img[y - 1, x] = 1                              # m01 = -1
    img[y - 8:y + 9, x + 5:x + 13] = 20            # symmetric in v: m10 = 20 * 17 * (5 + ... + 12), m01 += 0
    m10 = 20 * 17 * sum(range(5, 13))
    pl.append(Plant("angle_near_360", "angle", (0, x, y), ("exact", ref.fast_atan2_small(m10, -1))))
    pl.append(Plant("angle_near_360", "angle", (0, x, y), ("near", m10, -1)))
    return _done("angles", "detect", img, pl)


# ------------------------------------------------------------------------------------------ 1.4 cornerSubPix
CORNER_A = (80.3, 70.6)      # the analytic corner of subpix_ideal_corner
CORNER_B = (11.4, 60.3)      # a second one 11 px from the left edge (no staged neighbourhood there)


def _checker(img, cx, cy, r, lo=40.0, hi=200.0):
    """A 2 x 2 checker corner at (cx, cy), box-filtered over each pixel (pixel (x, y) covers x +- .5, y +- .5)."""
    for y in range(int(cy - r), int(cy + r) + 1):
        for x in range(int(cx - r), int(cx + r) + 1):
            fx = min(max(cx - (x - 0.5), 0.0), 1.0)     # the part of the pixel left of the corner
            fy = min(max(cy - (y - 0.5), 0.0), 1.0)
            img[y, x] = int(round(lo + (hi - lo) * (fx * (1 - fy) + (1 - fx) * fy)))


@functools.lru_cache(maxsize=None)
def subpix_image():
    img = _flat(60)
    _checker(img, *CORNER_A, 14)
    _checker(img, *CORNER_B, 8)
    t = math.tan(math.radians(35.0))
    for y in range(22):
        for x in range(96, 146):
            d = (t * (y - WEDGE_APEX[1]) - abs(x - WEDGE_APEX[0])) / math.hypot(1.0, t)      # > 0 inside the wedge
            img[y, x] = int(round(min(max(120 + 80 * d, 40), 200)))
    rng = np.random.default_rng(5)
    img[90:, 100:] = rng.integers(0, 256, (H1 - 90, W1 - 100), dtype=np.uint8)     # texture up to the lower right edges
    img[:24, :24] = rng.integers(0, 256, (24, 24), dtype=np.uint8)                   # and in the upper left corner
    img.setflags(write=False)
    return img


# starts in the texture, found once by running bird_ref.corner_subpix over 2000 seeded starts
# (rng 7, uniform over [104, 186] x [94, 154]) and keeping the first of each kind; tests/test_bird_cases.py asserts
# that the oracle walks the same path (_oracle_follows, the 39 / 41 iteration results)
SUBPIX_RESET = (167.60623168945312, 150.52952575683594)          # converges 5.2 px away in 28 iterations: put back
SUBPIX_40 = (149.38677978515625, 148.04917907714844)              # still moving after 40 iterations, 1.5 px away
WEDGE_APEX = (120.3, -2.6)   # two edges that meet above the image: the first step lands there


def _subpix():
    img = subpix_image()
    pts, pl = [], []

    def add(item, xy, **expect):
        pts.append(xy)
        pl.append(Plant(item, "subpix", len(pts) - 1, expect))

    add("subpix_flat_unchanged", (150.0, 40.0), exit=ref.SINGULAR, iters=1, unchanged=True)
    add("subpix_flat_unchanged", (40.25, 120.5), exit=ref.SINGULAR, iters=1, unchanged=True)
    for xy in ((80.0, 71.0), (80.5, 70.5), (83.3, 70.6), (77.5, 73.5)):      # integer (the 1e-4 clamp), .5, 3 px away
        add("subpix_ideal_corner", xy, exit=ref.EPS, analytic=CORNER_A, integer_start=xy == (80.0, 71.0))
    add("subpix_reset_over_5px", SUBPIX_RESET, reset=True, oracle_only=True)
    add("subpix_leaves_image", (120.0, 1.5), exit=ref.LEFT_IMAGE, iters=1, reset=False, outside=True)
    add("subpix_leaves_image", (119.5, 3.0), exit=ref.LEFT_IMAGE, iters=1, reset=True)
    add("subpix_border_replicate", (0.3, 0.2), inside_first=False)
    add("subpix_border_replicate", (W1 - 0.6, H1 - 0.4), inside_first=False)
    add("subpix_uncached_inside", (12.0, 61.0), exit=ref.EPS, analytic=CORNER_B, inside_first=True, uncached=True)
    add("subpix_uncached_inside", (10.5, 59.5), exit=ref.EPS, analytic=CORNER_B, inside_first=True, uncached=True)
    add("subpix_40_iterations", SUBPIX_40, exit=ref.MAX_ITER, iters=40, oracle_only=True)
    # the float32 of a converged float64 result: the first iteration moves less than eps
    (x, y), _, _ = ref.corner_subpix(img, (80.5, 70.5))
    add("subpix_eps_exit_first_iteration", (float(np.float32(x)), float(np.float32(y))), exit=ref.EPS, iters=1)
    return _done("subpix", "subpix", img, pl, pts=np.array(pts, np.float32))


# found the same way on the 320 x 240 texture (rng 9, uniform over [40, 280] x [40, 200]): the first start whose
# 13 x 13 patch stays inside the image on every iteration while it drifts out of the 32 x 32 neighbourhood of the start
# (first at iteration 21, 10.9 px away after 23, 38 iterations in all, then put back)
SUBPIX_LEAVES_CACHE = (86.82073211669922, 76.19386291503906)


def in_start_neighbourhood(start, ipx, ipy):
    """Whether a 13 x 13 patch (+ 1 for the bilinear tap) with first pixel (ipx, ipy) lies in the 32 x 32 pixels
    around the start point, [floor(s) - 15, floor(s) + 17) in x and y: the part k_bird_subpix stages once."""
    fx, fy = math.floor(start[0]), math.floor(start[1])
    return fx - 15 <= ipx and ipx + 13 < fx + 17 and fy - 15 <= ipy and ipy + 13 < fy + 17


def _subpix_texture():
    pts = np.array([SUBPIX_LEAVES_CACHE], np.float32)
    pl = [Plant("subpix_leaves_cache", "subpix", 0, dict(leaves_cache=True, reset=True, oracle_only=True))]
    return _done("subpix_texture", "subpix", noise_image(W8, H8, 12), pl, pts=pts)


def _subpix_flat():
    pts = np.array([(96.0, 80.0), (17.25, 9.5), (0.0, 0.0)], np.float32)
    pl = [Plant("subpix_flat_unchanged", "subpix", i, dict(exit=ref.SINGULAR, iters=1, unchanged=True)) for i in range(3)]
    return _done("subpix_flat", "subpix", _flat(77), pl, pts=pts)


# ------------------------------------------------------------------------------------------ 1.5 descriptors
def _kps(rows):
    k = np.zeros(len(rows), KP_DTYPE)
    for i, (x, y, angle, octave) in enumerate(rows):
        k[i] = (x, y, 31.0 * 1.2 ** octave, angle, 1.0, octave, -1)
    return k


@functools.lru_cache(maxsize=None)
def noise_image(w=W1, h=H1, seed=11):
    img = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    img.setflags(write=False)
    return img


def _desc_flat():
    k = _kps([(96, 80, 33.0, 0), (40.4, 50.6, 271.0, 0)])
    pl = [Plant("desc_flat_all_zero", "desc", i, dict(all_zero=True)) for i in range(2)]
    return _done("desc_flat", "compute", _flat(77), pl, kps=k)


def _desc_noise():
    img = noise_image()
    b = ref.blur(img)
    rows = [(96, 80, 0.0, 0), (96, 80, 90.0, 0), (60.4, 100.6, 0.0, 0), (131.5, 57.5, 90.0, 0)]
    pl = [Plant("desc_angle_0", "desc", 0, dict(ref=True)), Plant("desc_angle_90", "desc", 1, dict(ref=True)),
          Plant("desc_angle_0", "desc", 2, dict(ref=True)), Plant("desc_angle_90", "desc", 3, dict(ref=True))]
    # a pair whose second sample is one above the first (bit 1) and one whose second is one below (bit 0)
    found = {}
    for cx in range(40, 150, 7):
        _, v = ref.descriptor(b, cx, 75, 0.0)
        for want in (1, -1):
            p = np.flatnonzero(v[:, 1] - v[:, 0] == want)
            if want not in found and len(p):
                found[want] = (cx, int(p[0]))
    assert set(found) == {1, -1}
    for want, (cx, p) in sorted(found.items()):
        rows.append((cx, 75, 0.0, 0))
        pl.append(Plant("desc_pair_differs_by_one", "desc", len(rows) - 1, dict(ref=True, pair=p, bit=int(want == 1))))
    # border cull on the rounded position (half to even): 30 is out, 31 is in; W - 32 is in, W - 31 is out
    for x, y, kept in ((30.4, 80, False), (30.5, 80, False), (30.6, 80, True), (31.5, 80, True), (W1 - 31.6, 80, True),
                       (W1 - 31.4, 80, False), (96, 30.4, False), (96, 30.6, True), (96, H1 - 31.6, True),
                       (96, H1 - 31.4, False), (31, 31, True), (W1 - 32, H1 - 32, True), (30, 31, False)):
        rows.append((x, y, 0.0, 0))
        pl.append(Plant("desc_culled_by_border", "desc", len(rows) - 1, dict(kept=kept)))
    return _done("desc_noise", "compute", img, pl, kps=_kps(rows))


def _samples_outside(x, y, angle, octave):
    w, h, sc = ref.level_sizes(W8, H8, 8)[octave]
    cx, cy = int(np.rint(np.float32(x) / np.float32(sc))), int(np.rint(np.float32(y) / np.float32(sc)))
    ox, oy = ref.sample_offsets(angle, strict=False)
    return int(((cx + ox < 0) | (cx + ox >= w) | (cy + oy < 0) | (cy + oy >= h)).sum())


def _desc_roi():
    """Octave 5..7 keypoints 31..40 px from each edge and corner of a 320 x 240 texture: at level scale 2.49..3.58
    that is 9..16 level pixels, inside the pattern's reach of 13, so samples fall outside the level."""
    rows, pl = [], []
    angles = (0.0, 90.0, 180.0, 270.0, 45.7, 201.3, 333.0)
    n = 0
    for octave in (5, 6, 7):
        for d in (31, 36, 40):
            lo_x, hi_x, lo_y, hi_y = d, W8 - 1 - d, d, H8 - 1 - d
            for x, y, sides in ((lo_x, 120, 1), (hi_x, 120, 1), (160, lo_y, 1), (160, hi_y, 1), (lo_x, lo_y, 2),
                                (hi_x, lo_y, 2), (lo_x, hi_y, 2), (hi_x, hi_y, 2)):
                angle = angles[n % len(angles)]
                if d == 31:       # a plant: the first angle from there on at which a sample does leave the level
                    angle = next(a for a in angles[n % len(angles):] + angles if _samples_outside(x, y, a, octave))
                    pl.append(Plant("desc_outside_roi", "desc", len(rows), dict(sides=sides)))
                rows.append((x, y, angle, octave))
                n += 1
    return _done("desc_roi", "compute", noise_image(W8, H8, 12), pl, nfeat=2000, nlevels=8, kps=_kps(rows))


# ------------------------------------------------------------------------------------------ 1.6 blur
BLUR_W = 190
BLUR_PAIR = 1        # pattern pair (4, 2) / (7, -12): 14 px apart, so its first sample is on the flat field


def _half_search(x, y, w, h, flat, want_q, rng):
    """Three pixels within 3 px of (x, y) and their new values such that the 7 x 7 sum at (x, y) is exactly
    want_q * 65536 + 32768: seeded draws of two pixels and their values, evaluated at once through the blur's
    weights at (x, y); the third pixel's value is solved for."""
    k = ref.gauss_q8()
    wmap = collections.defaultdict(int)
    r101 = lambda p, n: -p if p < 0 else (2 * n - 2 - p if p >= n else p)
    for i in range(7):
        for j in range(7):
            wmap[(r101(x + j - 3, w), r101(y + i - 3, h))] += int(k[i] * k[j])
    pix = sorted(wmap)
    wts = np.array([wmap[p] for p in pix], np.int64)
    n = 200000
    idx = rng.integers(0, len(pix), (n, 3))
    dlt = rng.integers(-40, 120, (n, 3))
    # two pixels drawn, the third pixel's change solved for: kept when it is a whole number in range
    need = want_q * 65536 + 32768 - flat * int(k.sum()) ** 2 - (wts[idx[:, :2]] * dlt[:, :2]).sum(1)
    w3 = wts[idx[:, 2]]
    dlt[:, 2] = need // w3
    ok = ((need % w3 == 0) & (dlt[:, 2] >= -40) & (dlt[:, 2] < 120) & (idx[:, 0] != idx[:, 1]) &
          (idx[:, 1] != idx[:, 2]) & (idx[:, 0] != idx[:, 2]))
    hit = np.flatnonzero(ok)
    assert len(hit), "no exact half found at (%d, %d)" % (x, y)
    t = hit[0]
    return [(pix[i], flat + int(d)) for i, d in zip(idx[t], dlt[t])]


@functools.lru_cache(maxsize=None)
def _blur():
    """A flat field of 50 (its 7 x 7 sum is 50 * 257^2 = 50 * 65536 + 25650: blurred 50).  Three pixels are given an
    exact half: (60, 60) with quotient 50 (even: half-to-even gives 50, half-up would give 51), (110, 60) with
    quotient 51 (odd: 52 by both rules) and (189, 60) in the tail columns with quotient 50 (half-up: 51; half-to-even
    would give 50).  Each body pixel is the second sample of pattern pair BLUR_PAIR of a keypoint whose first sample
    lies on the untouched field, so the descriptor bit is val(50) < val(plant)."""
    img = _flat(50, BLUR_W, H1)
    rng = np.random.default_rng(21)
    pl, rows = [], []
    pat = ref.pattern()[BLUR_PAIR]
    for (x, y), q, val in (((60, 60), 50, 50), ((110, 60), 51, 52), ((BLUR_W - 1, 60), 50, 51)):
        for (px, py), v in _half_search(x, y, BLUR_W, H1, 50, q, rng):
            img[py, px] = v
        pl.append(Plant("blur_exact_half", "blur", (x, y), (q, val)))
        if x < (BLUR_W & ~3):
            rows.append((x - int(pat[2]), y - int(pat[3]), 0.0, 0))
            pl.append(Plant("blur_exact_half", "desc", len(rows) - 1, dict(ref=True, pair=BLUR_PAIR, bit=int(50 < val),
                                                   **({"other_rule": "half_up"} if q % 2 == 0 else {}))))
    return _done("blur", "compute", img, pl, kps=_kps(rows))


TAIL_LEVEL, TAIL_XY = 4, (152, 71)
TAIL_PAIR = 194      # at 90 degrees its second sample is at (+13, +1), its first at (-11, -1)
TAIL_FIRST_SEED = 1139


def _blur_tail():
    """A tail-column exact half that a descriptor can reach.  Level 4 of a 320-wide image is 154 wide (tail columns
    152, 153); the border cull acts on level-0 coordinates, so an octave-4 keypoint at level-0 x = 288 sits at level
    x = 139 and the pattern's 13-pixel arm reaches column 152.  The image is a flat field of 50 (every level is 50,
    blurred 50) with seeded noise of +-12 in columns 300..319; the seeds are tried in order until level 4 has the 7 x 7
    sum 50 * 65536 + 32768 at TAIL_XY (from seed 1000 the first is 1139, about a second; the builder starts there).
    Half-up gives 51, half-to-even would give 50; the keypoint's pair TAIL_PAIR compares it with the untouched field:
    bit = 50 < 51."""
    for seed in range(TAIL_FIRST_SEED, TAIL_FIRST_SEED + 2000):
        img = _flat(50, W8, H8)
        img[40:200, 300:] = 50 + np.random.default_rng(seed).integers(-12, 13, (160, 20))
        l4 = ref.pyramid(img, TAIL_LEVEL + 1)[TAIL_LEVEL]
        if int(ref.blur_sums(l4)[TAIL_XY[1], TAIL_XY[0]]) == 50 * 65536 + 32768:
            break
    else:
        raise AssertionError("no exact half at level %d %r" % (TAIL_LEVEL, TAIL_XY))
    ox, oy = ref.sample_offsets(90.0)
    cx, cy = TAIL_XY[0] - int(ox[2 * TAIL_PAIR + 1]), TAIL_XY[1] - int(oy[2 * TAIL_PAIR + 1])
    sc = ref.level_sizes(W8, H8, TAIL_LEVEL + 1)[TAIL_LEVEL][2]
    x0, y0 = W8 - 32, int(round(cy * sc))
    assert int(np.rint(np.float32(x0) / np.float32(sc))) == cx and int(np.rint(np.float32(y0) / np.float32(sc))) == cy
    pl = [Plant("blur_exact_half", "blur", TAIL_XY + (TAIL_LEVEL,), (50, 51)),
          Plant("blur_exact_half", "desc", 0, dict(ref=True, pair=TAIL_PAIR, bit=1, other_rule="half_even"))]
    return _done("blur_tail", "compute", img, pl, nfeat=2000, nlevels=8, kps=_kps([(x0, y0, 90.0, TAIL_LEVEL)]))


# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    cs = (_fast(), _fast255(), _nms(), _mask0(), _mask_pyr(), _footprint(), _harris(), _sel(3), _sel(5), _margin(),
          _angles(), _subpix(), _subpix_texture(), _subpix_flat(), _desc_flat(), _desc_noise(), _desc_roi(), _blur(),
          _blur_tail())
    return collections.OrderedDict((c.name, c) for c in cs)


def by_kind(kind):
    return [c for c in cases().values() if c.kind == kind]


def batch_frames():
    """Every 192 x 160 case (detect, cornerSubPix and compute images alike) and its mask (all 255 where the case has
    none): the batch test's frames."""
    cs = [c for c in cases().values() if c.img.shape == (H1, W1)]
    return cs, [c.img for c in cs], [c.mask if c.mask is not None else _flat(255) for c in cs]


# ------------------------------------------------------------------------------------------ plant checks
# Each returns [(item, detail)] for the plants a result does not show; the result may come from the oracle or the GPU.
def detect_failures(case, cands, kps):
    """cands: per level, a KP_DTYPE array (x, y level coordinates, class_id the FAST score); kps: detect()'s output."""
    bad = []
    scales = [s for _, _, s in ref.level_sizes(case.img.shape[1], case.img.shape[0], case.nlevels)]
    have = [{(int(c["x"]), int(c["y"])): int(c["class_id"]) for c in cl} for cl in cands]
    out = {(int(k["octave"]), float(k["x"]), float(k["y"])): k for k in kps}
    key = lambda l, x, y: (l, float(np.float32(x) * np.float32(scales[l])), float(np.float32(y) * np.float32(scales[l])))
    for p in case.plants:
        if p.what == "cand":
            l, x, y = p.where
            present, raw = p.expect
            if ((x, y) in have[l]) != present or (present and have[l][(x, y)] != raw):
                bad.append((p.item, (p.where, p.expect, have[l].get((x, y)))))
        elif p.what == "count":
            n = sum(key(*w) in out for w in p.where)
            if n != p.expect:
                bad.append((p.item, (p.where, p.expect, n)))
        elif p.what == "angle":
            k = out.get(key(*p.where))
            if k is None:
                bad.append((p.item, (p.where, "no keypoint")))
            elif p.expect[0] == "exact" and np.float32(k["angle"]).tobytes() != np.float32(p.expect[1]).tobytes():
                bad.append((p.item, (p.where, p.expect, float(k["angle"]))))
            elif p.expect[0] == "near" and abs(float(k["angle"]) - ref.angle_deg(*p.expect[1:])) > 0.3:
                bad.append((p.item, (p.where, p.expect, float(k["angle"]))))
        elif p.what == "harris":
            l, x, y = p.where
            r = [float(c["response"]) for c in cands[l] if (int(c["x"]), int(c["y"])) == (x, y)]
            if len(r) != 1 or (p.expect == "negative" and not r[0] < 0) or (p.expect == "above_2p24" and not r[0] > 0):
                bad.append((p.item, (p.where, p.expect, r)))
    return bad


def extract_failures(case, kps):
    bad = []
    for p in case.plants:
        if p.what == "extract":
            near = bool(len(kps)) and bool((np.maximum(np.abs(kps["x"] - p.where[0]), np.abs(kps["y"] - p.where[1])) < 1.5).any())
            if near != p.expect:
                bad.append((p.item, (p.where, p.expect)))
    return bad


def subpix_failures(case, out):
    """out: the refined points.  unchanged / reset: bit-identical to the start; analytic: within twice the measured
    distances of the analytic corner and of bird_ref's float64 result."""
    bad = []
    for p in case.plants:
        if p.what != "subpix":
            continue
        s, o, e = case.pts[p.where], out[p.where], p.expect
        if (e.get("unchanged") or e.get("reset")) and o.tobytes() != s.tobytes():
            bad.append((p.item, (s.tolist(), "moved to", o.tolist())))
        if e.get("reset") is False and o.tobytes() == s.tobytes():
            bad.append((p.item, (s.tolist(), "not moved")))
        if e.get("outside") and not (o[1] < 0):
            bad.append((p.item, (s.tolist(), "ends inside", o.tolist())))
        if "analytic" in e:
            r, _, _ = ref.corner_subpix(case.img, s)
            da = max(abs(o[0] - e["analytic"][0]), abs(o[1] - e["analytic"][1]))
            dr = max(abs(o[0] - r[0]), abs(o[1] - r[1]))
            if da > 2 * SUBPIX_ORACLE_TO_ANALYTIC or dr > 2 * SUBPIX_ORACLE_TO_REF:
                bad.append((p.item, (s.tolist(), o.tolist(), "analytic", da, "ref", dr)))
    return bad


def kept_inputs(case):
    """Indices of case.kps that compute() keeps (the border cull), in output order."""
    culled = {p.where for p in case.plants if p.what == "desc" and p.expect.get("kept") is False}
    return [i for i in range(len(case.kps)) if i not in culled]


@functools.lru_cache(maxsize=None)
def blurred(name, level=0, rule="opencv"):
    c = cases()[name]
    return ref.blur(ref.pyramid(c.img, level + 1)[level], rule)


def level_xy(case, k):
    """The rounded level position of keypoint k: cvRound(pt * (1 / scale))."""
    sc = np.float32(1) / np.float32(ref.level_sizes(case.img.shape[1], case.img.shape[0], int(k["octave"]) + 1)[-1][2])
    return int(np.rint(k["x"] * sc)), int(np.rint(k["y"] * sc))


def compute_failures(case, kps, desc):
    """kps, desc: compute()'s output for case.kps.  The kept set and order, the all-zero and the bird_ref descriptors
    (at the keypoint's level; samples inside it), the planted pair bits."""
    kept = kept_inputs(case)
    if len(kps) != len(kept) or any(kps[j]["x"] != case.kps[i]["x"] or kps[j]["y"] != case.kps[i]["y"]
                                    for j, i in enumerate(kept)):
        items = sorted({p.item for p in case.plants if p.what == "desc" and "kept" in p.expect})
        return [(it, ("kept set", len(kps), len(kept))) for it in items or ["kept set"]]
    row = {i: j for j, i in enumerate(kept)}
    bad = []
    for p in case.plants:
        if p.what != "desc" or p.where not in row:
            continue
        d, e, k = desc[row[p.where]], p.expect, case.kps[p.where]
        if e.get("all_zero") and d.any():
            bad.append((p.item, (p.where, d.tolist())))
        if e.get("ref"):
            want, _ = ref.descriptor(blurred(case.name, int(k["octave"])), *level_xy(case, k), float(k["angle"]))
            if not np.array_equal(d, want):
                bad.append((p.item, (p.where, "bits", np.flatnonzero(np.unpackbits(d ^ want, bitorder="little")).tolist())))
        if "pair" in e and (d[e["pair"] // 8] >> (e["pair"] % 8)) & 1 != e["bit"]:
            bad.append((p.item, (p.where, "pair", e["pair"], "bit", e["bit"])))
    return bad
