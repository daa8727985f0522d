"""Planted-decision cases of k_describe (csrc/extract_kernels.hip): frames whose keypoints are isolated dots (one
pixel DOT above the 16 pixels of its radius-3 circle, so FAST-9 fires there and nowhere around it) and whose 43 x 43
windows are the test's own bytes, built so that one named decision of IC_Angle, the blur or rBRIEF sits on its
boundary.  Everything else in a window is "weak": it differs from the background by at most minThFAST, so neither
FAST pass makes a keypoint of it.  One-level extractors (the pyramid is the image) except the `lvl1` family
(scaleFactor 2, two levels, level 0 made of constant 2 x 2 blocks: level 1 is the block values exactly).

A Plant names the keypoint, its level and position, the census items it is there for and a hand-written expectation
(`expect`, checked against the reference trace by realised()).  The builder's searches (a blur tie by a few weak
pixels, an angle that carries a pattern point into the scalar tail, moment pairs whose sample pixel depends on the
offset arithmetic) are exhaustive over small ranges in a fixed order: no randomness but the seeded textures.
SEARCH records what they found."""
import collections

import numpy as np

import describe_ref as R

INI_TH, MIN_TH = 20, 7
DOT = INI_TH + 1 + MIN_TH          # centre above the circle's maximum: weak pixels on the circle leave FAST firing
CIRCLE = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1),
          (-3, 0), (-3, -1), (-2, -2), (-1, -3)]
LO = 19   # the first keypoint coordinate: the cell grid starts at EDGE_THRESHOLD - 3 = 16 and cv::FAST skips 3 more
GRID = [(x, y) for y in (40, 88, 136, 184) for x in (40, 88, 136, 184, 232, 280)]   # 320 x 240, all interior

Plant = collections.namedtuple("Plant", "name level x y items expect")
Frame = collections.namedtuple("Frame", "name img levels nlevels scale nfeatures plants")

SEARCH = {}
_CACHE = {}


def bg_blur(b):
    """Blurred value of a constant region b before saturation: round(b * 257^2 / 65536) (no tie for any byte)."""
    return (b * 66049 + 32768) >> 16


class Canvas:
    def __init__(self, name, w, h, bg=100, level=0, nfeatures=500):
        self.name, self.level, self.nfeatures = name, level, nfeatures
        self.img = np.full((h, w), bg, np.int64) if np.isscalar(bg) else np.asarray(bg, np.int64).copy()
        self.plants = []

    def plant(self, name, x, y, mods=(), items=(), expect=None, dark=False, centre=None):
        for (u, v, d) in mods:
            self.img[y + v, x + u] += d
        ring = [self.img[y + dv, x + du] for (du, dv) in CIRCLE]
        self.img[y, x] = centre if centre is not None else (min(ring) - DOT if dark else max(ring) + DOT)
        self.plants.append(Plant(name, self.level, x, y, tuple(items), expect or {}))

    def fill(self, dark=False):
        """Flat dots on the free GRID positions (48 or more from every plant).  DistributeOctTree stops as soon as a
        round adds no node (:722), so two keypoints alone in one quadrant of the root would lose one: a frame needs
        keypoints in every quadrant for all of them to be kept."""
        h, w = self.img.shape
        for (x, y) in GRID:
            if x + 27 <= w and all(max(abs(x - p.x), abs(y - p.y)) >= 48 for p in self.plants):
                self.plant(f"filler_{x}_{y}", x, y, [], [], {}, dark=dark)
        return self

    def frame(self):
        assert self.img.min() >= 0 and self.img.max() <= 255, self.name
        lv = self.img.astype(np.uint8)
        if self.level == 0:
            return Frame(self.name, lv, [lv], 1, 1.2, self.nfeatures, self.plants)
        img = np.repeat(np.repeat(lv, 2, axis=0), 2, axis=1)
        return Frame(self.name, img, [img, lv], 2, 2.0, self.nfeatures, self.plants)


# ---- moments by weak pixels -------------------------------------------------------------------------------------

def in_patch(u, v):
    return abs(v) <= 15 and abs(u) <= R.UMAX[abs(v)]


def mods_moments(mods):
    m10 = sum(u * d for (u, v, d) in mods if in_patch(u, v))
    m01 = sum(v * d for (u, v, d) in mods if in_patch(u, v))
    return m10, m01


def _axis(r, carriers):
    """[(carrier, delta)] with sum weight * delta == r, |delta| <= MIN_TH, over carriers (weight, pixels): the
    heaviest first, weight 1 last."""
    out = []
    for c in sorted(carriers, key=lambda c: (-abs(c[0]), c[0], c[1])):
        if r == 0:
            break
        d = max(-MIN_TH, min(MIN_TH, int(r / c[0])))
        if d:
            out.append((c, d))
            r -= c[0] * d
    return out if r == 0 else None


def balance(mods, target, zones=()):
    """mods plus weak pixels so that the patch moments are target = (m10, m01): pixels on the two axes, and pairs
    mirrored in an axis ((n, k) and (n, -k) move m10 by 2n and m01 by nothing), all outside the zones (u, v, radius);
    None if they cannot carry the rest."""
    used = {(u, v) for (u, v, _) in mods}

    def free(u, v):
        return (in_patch(u, v) and (u, v) not in used
                and all(max(abs(u - zu), abs(v - zv)) > zr for (zu, zv, zr) in zones))
    m10, m01 = mods_moments(mods)
    ns = [n for n in range(-15, 16) if n]
    cx = [(n, ((n, 0),)) for n in ns if free(n, 0)]
    cx += [(2 * n, ((n, k), (n, -k))) for k in (5, 6, 7) for n in ns if abs(n) >= 5 and free(n, k) and free(n, -k)]
    ax = _axis(target[0] - m10, cx)
    if ax is None:
        return None
    used |= {p for (c, _) in ax for p in c[1]}
    cy = [(n, ((0, n),)) for n in ns if free(0, n)]
    cy += [(2 * n, ((k, n), (-k, n))) for k in (5, 6, 7) for n in ns if abs(n) >= 5 and free(k, n) and free(-k, n)]
    ay = _axis(target[1] - m01, cy)
    if ay is None:
        return None
    out = list(mods) + [(u, v, d) for (c, d) in ax + ay for (u, v) in c[1]]
    assert mods_moments(out) == tuple(target)
    return out


# ---- orientation ------------------------------------------------------------------------------------------------

def orientation_specs():
    """(name, mods, items, expect): expect m = (m10, m01) exactly, angle exactly where fastAtan2 is exact (c = 0),
    `near` the true angle in degrees (fastAtan2 is within 0.01 of it), `rel` an identity between two plants."""
    S = []
    S.append(("flat", [], ["angle0_flat"], dict(m=(0, 0), angle=0.0)))
    S.append(("symmetric", [(5, 2, 7), (-5, -2, 7), (-9, 4, -3), (9, -4, -3), (0, 12, 5), (0, -12, 5)],
              ["angle0_symmetric"], dict(m=(0, 0), angle=0.0)))
    for nm, (u, v), ang in [("axis0", (5, 0), 0.0), ("axis90", (0, 5), 90.0), ("axis180", (-5, 0), 180.0),
                            ("axis270", (0, -5), 270.0)]:
        S.append((nm, [(u, v, 1)], [nm], dict(m=(u, v), angle=ang)))
    for nm, (u, v), ang in [("diag45", (5, 5), 45.0), ("diag135", (-5, 5), 135.0), ("diag225", (-5, -5), 225.0),
                            ("diag315", (5, -5), 315.0)]:
        S.append((nm, [(u, v, 1)], [nm], dict(m=(u, v), near=ang)))
    S.append(("below360", [(15, 0, 7), (0, -1, 1)], ["below360"], dict(m=(105, -1), near=359.4543, below=360.0)))
    # |m10| = |m01| +- 1: the two sides of fastAtan2's |x| >= |y|
    S.append(("side_y49_x50", [(10, 10, 5), (0, -1, 1)], ["atan_x_ge_y"], dict(m=(50, 49), near=44.4213, below=45.0)))
    S.append(("side_y51_x50", [(10, 10, 5), (0, 1, 1)], ["atan_x_lt_y"], dict(m=(50, 51), near=45.5673, above=45.0)))
    S.append(("side_y50_x49", [(10, 10, 5), (-1, 0, 1)], ["atan_x_lt_y"], dict(m=(49, 50), near=45.5787, above=45.0)))
    S.append(("side_y50_x51", [(10, 10, 5), (1, 0, 1)], ["atan_x_ge_y"], dict(m=(51, 50), near=44.4327, below=45.0)))
    # every byte of the mask table: row v, both ends, the last pixel inside and the first outside; the base pixel
    # (0, 1, +1) makes the "nothing counted" angle 90 and not 0, which (+umax, 0) would give too
    for v in range(-15, 16):
        um = R.UMAX[abs(v)]
        for sg, sn in ((1, "p"), (-1, "n")):
            S.append((f"mask_in_v{v}{sn}", [(0, 1, 1), (sg * um, v, 7)], [f"mask_in_v{v}{sn}"],
                      dict(m=(7 * sg * um, 7 * v + 1), near=float(np.degrees(np.arctan2(7 * v + 1, 7 * sg * um)) % 360))))
            S.append((f"mask_out_v{v}{sn}", [(0, 1, 1), (sg * (um + 1), v, 7)], [f"mask_out_v{v}{sn}"],
                      dict(m=(0, 1), angle=90.0)))
    return S


def orientation_frames():
    specs = orientation_specs()
    out = []
    for f0 in range(0, len(specs), len(GRID)):
        c = Canvas(f"ori{f0 // len(GRID)}", 320, 240)
        for (nm, mods, items, exp), (x, y) in zip(specs[f0:f0 + len(GRID)], GRID):
            c.plant(nm, x, y, mods, items, exp)
        out.append(c.frame())
    # the largest moments: a 0 | 255 edge through the keypoints (a dark centre under nine bright circle pixels)
    half = sum(um * (um + 1) // 2 for um in (R.UMAX[abs(v)] for v in range(-15, 16)))
    bg = np.zeros((240, 320), np.int64)
    bg[:, 160:] = 255
    c = Canvas("max_m10", 320, 240, bg)
    for y in (40, 88, 136, 184):
        c.plant(f"max_m10_y{y}", 160, y, [], ["max_m10"], dict(m=(255 * half, 0), angle=0.0), centre=128)
    out.append(c.frame())
    bg = np.zeros((240, 320), np.int64)
    bg[120:, :] = 255
    c = Canvas("max_m01", 320, 240, bg)
    vsum = sum(v * (2 * R.UMAX[v] + 1) for v in range(1, 16))
    for x in (40, 88, 136, 184, 232, 280):
        c.plant(f"max_m01_x{x}", x, 120, [], ["max_m01"], dict(m=(0, 255 * vsum), angle=90.0), centre=128)
    out.append(c.frame())
    return out


# ---- window forms and edges -------------------------------------------------------------------------------------

def window_frame(w, h, level=0, name=None):
    """A seeded weak texture (96..103) and a full-range one in the outer 16 pixels, so the reflected rows and columns
    differ from replicate and from the neighbouring row; one 43 x 43 patch pasted at x = 0, 1, 2, 3 (mod 4) and both parities of y; dots on both
    sides of every clause of the interior test and at the extreme positions."""
    rng = np.random.default_rng(20240 + w * 1000 + h)
    c = Canvas(name or f"win{w}x{h}", w, h, rng.integers(96, 104, (h, w)), level, 500 if level == 0 else 300)
    patch = np.random.default_rng(7).integers(96, 104, (43, 43))
    if level == 0:
        # FAST never reads the outer 16 pixels (its cells start at EDGE_THRESHOLD - 3), the moments and the blur of
        # the extreme keypoints do: full-range bytes there, so a wrong border rule moves sums by whole grey levels
        strong = rng.integers(0, 256, (h, w))
        inner = np.zeros((h, w), bool)
        inner[16:h - 16, 16:w - 16] = True
        c.img = np.where(inner, c.img, strong)
        for y in (64, 113):
            for x in (64, 113, 162, 211):
                c.img[y - 21:y + 22, x - 21:x + 22] = patch
                c.plant(f"shift_x{x % 4}_y{y % 2}", x, y, [], [f"sh{x % 4}", f"ypar{y % 2}"], dict(group="shift"))
        edges = [("x20", 20, 160), ("x21", 21, 208), ("xw-27", w - 27, 160), ("xw-26", w - 26, 208),
                 ("y20", 100, 20), ("y21", 160, 21), ("yh-22", 100, h - 22), ("yh-21", 160, h - 21),
                 ("top", 220, LO), ("bottom", 220, h - 1 - LO), ("left", LO, 112), ("right", w - 1 - LO, 112),
                 ("inner", 150, 176)]
    else:
        edges = [("inner_a", 64, 60), ("inner_b", 112, 60)]
    edges += [("corner_tl", LO, LO), ("corner_tr", w - 1 - LO, LO), ("corner_bl", LO, h - 1 - LO),
              ("corner_br", w - 1 - LO, h - 1 - LO)]
    for nm, x, y in edges:
        inter = x >= 21 and x + 27 <= w and y >= 21 and y + 21 < h
        c.plant(nm, x, y, [], ["edge_" + nm], dict(interior_clauses=inter))
    return c.frame()


# ---- blur values ------------------------------------------------------------------------------------------------

def const_frame():
    """Bands of 0, 255, 127, 128 and a 127 / 128 checkerboard, 64 px each (a window is 43): the ^0x80 operands and
    the 128 * 257 accumulator bias at their ends; the largest row sum, 255 * 257 = 65535, in the second band."""
    bg = np.zeros((240, 320), np.int64)
    yy, xx = np.mgrid[0:240, 0:64]
    for i, b in enumerate((0, 255, 127, 128)):
        bg[:, 64 * i:64 * i + 64] = b
    bg[:, 256:320] = 127 + ((xx + yy) & 1)
    c = Canvas("const", 320, 240, bg)
    for i, b in enumerate((0, 255, 127, 128, "checker")):
        for y in (40, 88, 136, 184):
            exp = dict(far_val=bg_blur(b)) if b != "checker" else dict(far_vals=(128, 129))
            c.plant(f"const{b}_y{y}", 32 + 64 * i, y, [], [f"const{b}", "equal_bit0"], exp, dark=(b == 255))
    return c.frame()


SAT_PAIRS = {(255, 256): 0, (256, 257): 0, (255, 255): 0, (254, 257): 1}   # saturate_cast: 256, 257 compare as 255


def saturation_frame():
    """A 255 plateau with a 253 or 248 region starting u0 columns (or rows) from the keypoint: the blurred values
    run 257, 256, 255 (253 blurs to 255) or 257 ... 250 across the step.  The search keeps the fewest steps whose test pairs show every pair of
    SAT_PAIRS before saturation."""
    found, chosen = {}, []
    cands = [(ax, u0, sg, low) for low in (253, 248) for u0 in range(4, 13) for ax in (0, 1) for sg in (1, -1)]
    for (ax, u0, sg, low) in cands:
        win = np.full((64, 64), 255, np.int64)
        yy, xx = np.mgrid[0:64, 0:64] - 32
        win[(sg * (xx if ax == 0 else yy)) >= u0] = low
        win[32, 32] = min(win[32 + dv, 32 + du] for (du, dv) in CIRCLE) - DOT
        t = R.describe(win.astype(np.uint8), [(32, 32)])[0]
        have = {(int(a), int(b)) for a, b in zip(t.val[0::2], t.val[1::2])} & set(SAT_PAIRS)
        if have - set(found):
            chosen.append((ax, u0, sg, low, sorted(have - set(found))))
            for p in have:
                found.setdefault(p, (ax, u0, sg, low))
        if len(found) == len(SAT_PAIRS):
            break
    SEARCH["saturation"] = dict(steps_tried=len(cands), pairs_found=sorted(found), plants=len(chosen))
    c = Canvas("sat", 320, 240, 255)
    for (ax, u0, sg, low, pairs), (x, y) in zip(chosen, GRID):
        mods = [(u, v, low - 255) for u in range(-21, 22) for v in range(-21, 22) if sg * (u if ax == 0 else v) >= u0]
        c.plant(f"sat_{low}_ax{ax}_u{sg * u0}", x, y, mods, [f"sat_{a}_{b}" for a, b in pairs],
                dict(pairs={p: SAT_PAIRS[p] for p in pairs}), dark=True)
    return c.fill(dark=True).frame()


def column_weights(sx, w):
    """{du: weight} of the image columns sx + du under a sample at column sx of a level w wide (REFLECT_101 folds the
    taps past the border back inside)."""
    out = {}
    for t in range(-3, 4):
        cx = sx + t
        cx = -cx if cx < 0 else (2 * w - 2 - cx if cx >= w else cx)
        out[cx - sx] = out.get(cx - sx, 0) + int(R.K[t + 3])
    return out


def tie_mods(b, want_odd_q, sx, w):
    """Weak pixels around a sample at column sx on background b that make its blur sum S = q * 65536 + 32768 with q
    of the wanted parity: (mods relative to the sample, q), or None.  Five weights, every delta in -7..7, the
    smallest sum of |delta| among the first matches wins."""
    key = ("tie", b, want_odd_q, min(sx, 3), min(w - 1 - sx, 3))
    if key not in _CACHE:
        _CACHE[key] = _tie_mods(b, want_odd_q, sx, w)
    return _CACHE[key]


def _tie_mods(b, want_odd_q, sx, w):
    cw = column_weights(sx, w)
    pos = [(du, dv) for du in sorted(cw, key=lambda d: (abs(d), d)) for dv in (0, 1, 2, 3)]
    wts, seen = [], set()
    for (du, dv) in pos:
        wt = cw[du] * int(R.K[dv + 3])
        if wt not in seen:
            seen.add(wt)
            wts.append((du, dv, wt))
    A, Bw = wts[0:8:2][:4], wts[1:9:2][:5]
    base = b * 66049
    q0 = (base - 32768 + 65535) >> 16
    d = np.arange(-MIN_TH, MIN_TH + 1)

    def sums(ws):
        g = np.meshgrid(*[d] * len(ws), indexing="ij")
        return sum(gi * p[2] for gi, p in zip(g, ws)).ravel(), np.stack([gi.ravel() for gi in g], axis=1)
    sa, da = sums(A)
    sb, db = sums(Bw)
    order = np.argsort(sb, kind="stable")
    sbs = sb[order]
    for q in sorted((q0, q0 + 1, q0 - 1), key=lambda q: abs(q * 65536 + 32768 - base)):
        if (q & 1) != int(want_odd_q):
            continue
        T = q * 65536 + 32768 - base
        at = np.searchsorted(sbs, T - sa)
        ok = (at < len(sbs)) & (sbs[np.minimum(at, len(sbs) - 1)] == T - sa)
        if ok.any():
            ia = np.flatnonzero(ok)
            cost = np.abs(da[ia]).sum(axis=1) + np.abs(db[order[at[ia]]]).sum(axis=1)
            k = ia[np.argmin(cost)]
            deltas = list(da[k]) + list(db[order[at[k]]])
            return [(p[0], p[1], int(dl)) for p, dl in zip(A + Bw, deltas) if dl], q
    return None


def _far(ox, oy, j):
    """Point j's sample and its partner's are 7 or more apart (their 7 x 7 blur supports, and the weak pixels planted
    within 3 of either, do not meet) and each 4 or more from the keypoint (the dot reaches neither support)."""
    p = j ^ 1
    return (max(abs(ox[j] - ox[p]), abs(oy[j] - oy[p])) >= 7 and max(abs(ox[j]), abs(oy[j])) >= 4
            and max(abs(ox[p]), abs(oy[p])) >= 4)


def _far_pairs(ox, oy, want_odd_j):
    return [j for j in range(int(want_odd_j), 512, 2) if _far(ox, oy, j)]


def tie_plant(c, name, x, y, b, w, target, j, ox, oy, odd_q, partner_mods, items, where, bit):
    """A tie at pattern point j's sample of keypoint (x, y), moments balanced to `target`; False if no weak pixels
    make the tie or carry the moments."""
    p = j ^ 1
    tm = tie_mods(b, odd_q, x + int(ox[j]), w)
    if tm is None:
        return False
    mods = [(int(ox[j]) + du, int(oy[j]) + dv, d) for (du, dv, d) in tm[0]]
    mods += [(int(ox[p]) + du, int(oy[p]) + dv, d) for (du, dv, d) in partner_mods]
    mods = balance(mods, target, [(int(ox[j]), int(oy[j]), 3), (int(ox[p]), int(oy[p]), 3), (0, 0, 0)])
    if mods is None:
        return False
    q = tm[1]
    assert partner_mods or bg_blur(b) == (q if odd_q else q + 1), (b, q)
    tie_val = q + 1 if (where == "tail" or odd_q) else q
    part_val = (q + 1) if not partner_mods and not odd_q else q
    c.plant(name, x, y, mods, list(items) + ["oneapart_bit1"], dict(m=target, tie=(j, q, where), vals={j: tie_val, p: part_val},
                                          bits={j // 2: bit}))
    return True


def tie_body_frame():
    """Blur ties in the SSE2 body at angle 0 (m01 = m10 = 0: the samples are the pattern offsets).  Left band,
    background 64: S = 64 * 65536 + 32768 at point 2t's sample, the clean partner blurs to 65: half-even gives 64 and
    bit 1, half-up 65 and bit 0.  Right band, background 63: S = 63 * 65536 + 32768 at point 2t + 1's sample, the
    clean partner blurs to 63: both roundings give 64 and bit 1; dropping the parity term gives 63 and bit 0."""
    bg = np.full((240, 320), 64, np.int64)
    bg[:, 160:] = 63
    c = Canvas("tie_body", 320, 240, bg)
    ox, oy, _, _ = R.sample_offsets(R.f32(0.0))
    n = {}
    for odd_q, b, xs in ((False, 64, (40, 88)), (True, 63, (232, 280))):
        js = _far_pairs(ox, oy, odd_q)
        k = 0
        for x in xs:
            for y in (40, 88, 136, 184):
                while k < len(js) and not tie_plant(c, f"tie_{'odd' if odd_q else 'even'}_j{js[k]}", x, y, b, 320,
                                                    (0, 0), js[k], ox, oy, odd_q, [],
                                                    ["tie_odd_body" if odd_q else "tie_even_body"], "body", 1):
                    k += 1
                k += 1
        n["odd" if odd_q else "even"] = sum(1 for p in c.plants if ("odd" in p.name) == odd_q)
    SEARCH["tie_body"] = n
    return c.frame()


MOMENT_RANGE = 40

# Moment pairs (m10, m01) kept from wide_search(seed=1, n=400000, m=1500): 363,503 distinct angles of random integer
# moments |m| <= 1500 (what balance() can carry on the two axes is 7 * 2 * (1 + .. + 15) = 1680 each).  28 samples at
# 14 angles move under uncontracted offsets, 80 at 34 angles under cvRound half-away, 2 at one angle under correctly
# rounded trig.  Listed: every fma and trig angle, and the cvround angles with a sample whose test pair is apart.
WIDE_MOMENTS = {
    "fma": [(89, -783), (-982, -1369), (912, -781), (-602, 1416), (-1488, -953), (1372, 851), (1252, 1020),
            (1291, -119), (1076, -935), (1072, -1183), (-30, -785), (505, -1484), (162, 674), (-169, -880),
            (-643, 948)],
    "cvround": [(-97, -536), (1048, 1357), (-885, -406), (869, 1029), (1252, 1020), (-755, 589), (-765, 939),
                (1439, 592), (1076, -935), (406, -885), (-866, -1369), (505, -1484), (-1451, 900), (-244, -391),
                (-1290, 280), (74, -1313), (-1215, 67), (161, -394)],
    "trig": [(1252, 1020)],
}


def wide_search(seed=1, n=400000, m=1500):
    """The search WIDE_MOMENTS was kept from (about a minute; not run by the suite): per alternative rule the
    (m10, m01, point) whose sample pixel moves, over the distinct angles of n seeded random moment pairs |m| <= m."""
    rng = np.random.default_rng(seed)
    m10, m01 = rng.integers(-m, m + 1, n), rng.integers(-m, m + 1, n)
    ang = R.fast_atan2(m01.astype(R.f32), m10.astype(R.f32))
    _, first = np.unique(ang, return_index=True)
    first.sort()
    m10, m01, ang = m10[first], m01[first], ang[first]
    pat = R.pattern_points()
    out = {k: [] for k in OFFSET_ALTS}
    out["angles"] = len(ang)
    for i in range(0, len(ang), 4096):
        ox, oy, _, _ = R.sample_offsets(ang[i:i + 4096], R.PINNED, pat)
        for kind, alt in OFFSET_ALTS.items():
            ox2, oy2, _, _ = R.sample_offsets(ang[i:i + 4096], alt, pat)
            out[kind] += [(int(m10[i + a]), int(m01[i + a]), int(j)) for (a, j) in np.argwhere((ox != ox2) | (oy != oy2))]
    return out


def _all_offsets(rules):
    """(ox, oy, a, b) of every angle of _angles() under `rules`, in chunks (int16 offsets)."""
    key = ("off", rules)
    if key not in _CACHE:
        angs = _angles()[2]
        parts = [R.sample_offsets(angs[i:i + 2048], rules) for i in range(0, len(angs), 2048)]
        _CACHE[key] = (np.concatenate([p[0] for p in parts]).astype(np.int16),
                       np.concatenate([p[1] for p in parts]).astype(np.int16),
                       np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]))
    return _CACHE[key]


def _angles(rng=MOMENT_RANGE):
    """Distinct fastAtan2 angles of the integer moment pairs |m| <= rng and of WIDE_MOMENTS, with the first pair that
    gives each (the small pairs first)."""
    if "angles" in _CACHE:
        return _CACHE["angles"]
    m = np.arange(-rng, rng + 1)
    m10, m01 = [a.ravel() for a in np.meshgrid(m, m, indexing="ij")]
    keep = (m10 != 0) | (m01 != 0)
    m10, m01 = m10[keep], m01[keep]
    order = np.argsort(np.abs(m10) + np.abs(m01), kind="stable")
    wide = np.array(sorted({p for v in WIDE_MOMENTS.values() for p in v}, key=lambda p: (abs(p[0]) + abs(p[1]), p)))
    m10, m01 = np.concatenate([m10[order], wide[:, 0]]), np.concatenate([m01[order], wide[:, 1]])
    ang = R.fast_atan2(m01.astype(R.f32), m10.astype(R.f32))
    _, first = np.unique(ang, return_index=True)
    first.sort()
    _CACHE["angles"] = (m10[first], m01[first], ang[first])
    return _CACHE["angles"]


def tail_frames():
    """w = 321, 322, 323: keypoints at x = w - 20 and w - 21 (the last two columns FAST reaches) rotated (moments by
    weak pixels) so that a far pattern point's sample lands on column xsimd - 1 (half-even: tie under point 2t, clean partner) or xsimd (half-up: tie
    under point 2t + 1, partner one lower).  Background 64, even quotient: the two roundings differ."""
    m10s, m01s, angs = _angles()
    OX, OY, _, _ = _all_offsets(R.PINNED)
    out, report = [], {}
    for w in (321, 322, 323):
        xsimd = w & ~3
        c = Canvas(f"tail{w}", w, 240, 64)
        for x in (w - 1 - LO, w - 2 - LO):
            for where, col in (("body", xsimd - 1), ("tail", xsimd)):
                want, done = col - x, False
                odd_j = where == "tail"
                reach = np.argwhere(OX[:, int(odd_j)::2] == want)
                tried = 0
                for (ai, jj) in reach[:2000]:
                    j = 2 * int(jj) + int(odd_j)
                    if not _far(OX[ai], OY[ai], j):
                        continue
                    tried += 1
                    y = 40 + 48 * (len(c.plants) % 4)
                    done = tie_plant(c, f"tail_{where}_x{x - w}_j{j}", x, y, 64, w, (int(m10s[ai]), int(m01s[ai])), j,
                                     OX[ai], OY[ai], False, [(0, 0, -1)] if odd_j else [],
                                     [f"tie_{where}_w{w % 4}"], where, 1)
                    if done:
                        break
                report[f"w{w}_x{x - w}_{where}"] = dict(offset=int(want), angles_reaching=int(len(reach)), planted=done)
        out.append(c)
    SEARCH["tail"] = report
    return [c.fill().frame() for c in out if c.plants]


# ---- sample offsets ---------------------------------------------------------------------------------------------

OFFSET_ALTS = {"fma": R.PINNED._replace(fma=False), "trig": R.PINNED._replace(trig="cr"),
               "cvround": R.PINNED._replace(cvround="away")}


def offset_frames():
    """Moment pairs for which one of the 512 samples falls on a different pixel under uncontracted offsets, correctly
    rounded trig or cvRound half-away.  The two candidate pixels (one apart along x or y) get blurred values 100 and
    102 by a weak ramp (-7, -5 .. +7 across them, 7 wide: its blur is exactly -1 and +1 there), the partner keeps the
    background's 101; the pinned rule reads the side that makes the bit 1."""
    from kf_projection_ref import fmaf, f32
    m10s, m01s, angs = _angles()
    OX, OY, A, B = _all_offsets(R.PINNED)
    pat = R.pattern_points()
    out = []
    for kind, alt in OFFSET_ALTS.items():
        ox2, oy2, _, _ = _all_offsets(alt)
        diff = np.argwhere((OX != ox2) | (OY != oy2))
        c = Canvas(f"off_{kind}", 320, 240, 100)
        usable = 0
        for (ai, j) in diff:
            if len(c.plants) == 8:
                break
            ai, j = int(ai), int(j)
            pa, pb = (int(OX[ai, j]), int(OY[ai, j])), (int(ox2[ai, j]), int(oy2[ai, j]))
            p = j ^ 1
            pp = (int(OX[ai, p]), int(OY[ai, p]))
            if abs(pa[0] - pb[0]) + abs(pa[1] - pb[1]) != 1 or (int(ox2[ai, p]), int(oy2[ai, p])) != pp:
                continue
            # the finalist's pinned pixel under the exact float32 fma
            px, py = pat[j]
            ex = fmaf(px, A[ai], -f32(py * B[ai]))
            ey = fmaf(px, B[ai], f32(py * A[ai]))
            assert (int(np.rint(ex)), int(np.rint(ey))) == pa, (ai, j)
            lo, hi = (pa, pb) if j % 2 == 0 else (pb, pa)       # point 2t low or point 2t + 1 high: bit 1
            e = (hi[0] - lo[0], hi[1] - lo[1])
            # the ramp inside the window and off the dot, the dot outside the two candidates' and the partner's blur
            # supports, the partner's support off the ramp; if the full ramp (7 rows across) meets the partner's
            # support, the outermost row on one side is left out (its tap weighs 18 of 257: the ramp then blurs to
            # -+239/257, and 100 and 102 still)
            if min(max(abs(q[0]), abs(q[1])) for q in (lo, hi, pp)) < 4:
                continue
            psup = {(pp[0] + du, pp[1] + dv) for du in range(-3, 4) for dv in range(-3, 4)}
            mods = None
            for (s0, s1) in ((-3, 3), (-3, 2), (-2, 3)):
                cand = [(lo[0] + t * e[0] + sp * e[1], lo[1] + t * e[1] + sp * e[0], -1 + 2 * t)
                        for t in range(-3, 5) for sp in range(s0, s1 + 1)]
                ramp = {(u, v) for (u, v, _) in cand}
                if all(max(abs(u), abs(v)) <= 21 for (u, v) in ramp) and (0, 0) not in ramp and not (psup & ramp):
                    mods, wsum = cand, 257 - 18 * (6 - (s1 - s0))
                    break
            if mods is None:
                continue
            usable += 1
            zones = [(lo[0], lo[1], 3), (hi[0], hi[1], 3), (pp[0], pp[1], 3), (0, 0, 0)]
            mods = balance(mods, (int(m10s[ai]), int(m01s[ai])), zones)
            if mods is None:
                continue
            x, y = GRID[3 * len(c.plants)]
            c.plant(f"off_{kind}_m{int(m10s[ai])}_{int(m01s[ai])}_j{j}", x, y, mods, [f"offset_{kind}"],
                    dict(m=(int(m10s[ai]), int(m01s[ai])), pixel={j: pa}, alt_pixel={j: pb},
                         vals={j: ((25700 + (-wsum if j % 2 == 0 else wsum)) * 257 + 32768) >> 16, p: 101},
                         bits={j // 2: 1}))
        SEARCH[f"offset_{kind}"] = dict(angles=int(len(angs)), differing_samples=int(len(diff)),
                                        differing_angles=int(len(set(diff[:, 0].tolist()))), usable_seen=usable,
                                        planted=len(c.plants))
        if c.plants:
            out.append(c.fill().frame())
    return out


_FRAMES = None


def frames():
    global _FRAMES
    if _FRAMES is None:
        f = orientation_frames()
        f += [window_frame(w, 240) for w in (320, 321, 322, 323)]
        f += [const_frame(), saturation_frame(), tie_body_frame()]
        f += tail_frames()
        f += offset_frames()
        f += [window_frame(160, 120, level=1, name="lvl1")]
        _FRAMES = f
    return _FRAMES


# every census item the suite must realise (test_describe_cases.py: each is carried by a planted keypoint)
def census_items():
    items = ["angle0_flat", "angle0_symmetric", "axis0", "axis90", "axis180", "axis270", "diag45", "diag135",
             "diag225", "diag315", "below360", "atan_x_ge_y", "atan_x_lt_y", "max_m10", "max_m01"]
    items += [f"mask_{io}_v{v}{s}" for io in ("in", "out") for v in range(-15, 16) for s in "pn"]
    items += [f"sh{i}" for i in range(4)] + ["ypar0", "ypar1"]
    items += ["edge_" + e for e in ("x20", "x21", "xw-27", "xw-26", "y20", "y21", "yh-22", "yh-21", "top", "bottom",
                                    "left", "right", "corner_tl", "corner_tr", "corner_bl", "corner_br")]
    items += [f"const{b}" for b in (0, 255, 127, 128, "checker")] + ["equal_bit0", "oneapart_bit1"]
    items += [f"sat_{a}_{b}" for (a, b) in SAT_PAIRS]
    items += ["tie_even_body", "tie_odd_body"]
    items += [f"tie_{wh}_w{r}" for wh in ("body", "tail") for r in (1, 2, 3)]
    items += [f"offset_{k}" for k in OFFSET_ALTS]
    return items


def realised(frame, plant, t):
    """The plant's hand-written expectation against the reference trace t: a list of what does not hold."""
    e, bad = plant.expect, []
    w = frame.levels[plant.level].shape[1]
    if "m" in e and (t.m10, t.m01) != tuple(e["m"]):
        bad.append(("moments", (t.m10, t.m01), e["m"]))
    if "angle" in e and float(t.angle) != e["angle"]:
        bad.append(("angle", float(t.angle), e["angle"]))
    if "near" in e and abs(float(t.angle) - e["near"]) > 0.011:
        bad.append(("near", float(t.angle), e["near"]))
    if "below" in e and not float(t.angle) < e["below"]:
        bad.append(("below", float(t.angle)))
    if "above" in e and not float(t.angle) > e["above"]:
        bad.append(("above", float(t.angle)))
    far = np.maximum(np.abs(t.ox), np.abs(t.oy)) >= 4
    if "far_val" in e and not (t.val[far] == e["far_val"]).all():
        bad.append(("far_val", sorted(set(t.val[far].tolist())), e["far_val"]))
    if "far_val" in e and (not (far[0::2] & far[1::2]).any() or t.bits[far[0::2] & far[1::2]].any()):
        bad.append(("equal values must give bit 0", int(t.bits[far[0::2] & far[1::2]].sum())))
    if "far_vals" in e and not set(t.val[far].tolist()) <= set(e["far_vals"]):
        bad.append(("far_vals", sorted(set(t.val[far].tolist()))))
    for p, bit in e.get("pairs", {}).items():
        hit = [i for i in range(256) if (int(t.val[2 * i]), int(t.val[2 * i + 1])) == p]
        if not hit or any(int(t.bits[i]) != bit for i in hit):
            bad.append(("pair", p, len(hit)))
    if "tie" in e:
        j, q, where = e["tie"]
        if int(t.S[j]) != q * 65536 + 32768 or bool(t.tail[j]) != (where == "tail"):
            bad.append(("tie", j, int(t.S[j]) - q * 65536, bool(t.tail[j])))
        if where != "body" or "tail" in plant.name:   # the planted column is the first of the tail or the last before it
            col = plant.x + int(t.ox[j])
            if col != (w & ~3) - (where == "body"):
                bad.append(("tail column", col, w & ~3))
    for j, px in e.get("pixel", {}).items():
        if (int(t.ox[j]), int(t.oy[j])) != tuple(px):
            bad.append(("pixel", j, (int(t.ox[j]), int(t.oy[j])), px))
    for j, v in e.get("vals", {}).items():
        if int(t.val[j]) != v:
            bad.append(("val", j, int(t.val[j]), v))
    for i, bit in e.get("bits", {}).items():
        if int(t.bits[i]) != bit:
            bad.append(("bit", i, int(t.bits[i]), bit))
    return bad


def border_sides(frame, plant, t):
    """The level borders that the 7 x 7 blur support of some sample of this keypoint crosses (REFLECT_101 live)."""
    h, w = frame.levels[plant.level].shape
    sx, sy = plant.x + t.ox, plant.y + t.oy
    return {n for n, c in (("left", sx - 3 < 0), ("right", sx + 3 >= w), ("top", sy - 3 < 0), ("bottom", sy + 3 >= h))
            if c.any()}


# Census items no constructible input reached, with the search's bounds.  test_describe_cases.py
# asserts that exactly these are missing, so a search that reaches one has to move it out of this table.
UNREACHED = {
    "tie_tail_w1": "w % 4 = 1: the tail is column w - 1, 19 from the last keypoint column w - 20; the longest pattern "
                   "point is 18.385, so no angle samples further than 18",
}
