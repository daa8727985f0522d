"""Named, deterministic inputs that put every decision of Frame::ComputeStereoMatches (Frame.cc:662-836) at its
edge.  Pure numpy: tests/test_stereo_cases.py checks on the CPU that tests/stereo_ref.py and the oracle agree on every
case and that every planted decision is realised in the reference trace; tests/test_gpu_stereo_cases.py runs the same
arrays through k_stereo_bucket / k_stereo / k_stereo_cut.

The keypoints and descriptors are planted, not extracted.  The right image is the left image moved SHIFT pixels to the
left, so a right keypoint SHIFT pixels left of a left keypoint is a true partner: at octave 0 its window distance at
offset 0 is exactly 0, and plant_sad() then raises it to a chosen value by editing a few non-centre pixels of the
right window.  A descriptor is 256 random bits; a partner at Hamming distance d has exactly d of them flipped.  A
decoy is a right keypoint at distance 0 that a gate (row band, octave, u range) must exclude; it sits at least 12
scaled pixels from the partner, so taking it moves the window search elsewhere and changes mvuRight.

Each Plant names one item of the census (ITEMS) and what the reference trace must show for left keypoint iL; None
means "not pinned here".  A case is built once and never modified."""
import collections
import functools

import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
f32 = np.float32
SHIFT = 8

Case = collections.namedtuple("Case", "name left right kl dl kr dr mb mbf params plants")
Plant = collections.namedtuple("Plant", "item iL best_idx best_dist outcome bestinc sad visible")

ACCEPTED, CLAMPED, CUT = "accepted", "clamped to 0.01", "cut"
DIST_HIGH, NO_CANDIDATE, WINDOW_OFF = "dist >= 75", "no candidate", "window off the image"
BEST_AT_L, DISPARITY_RANGE = "best at +-L", "disparity out of range"

# the census: every item must be planted by some case and realised in the reference trace
ITEMS = (
    "tie_lower_ir", "tie_lower_ir_later_row", "tie_beyond_64",
    "dist_0", "dist_74", "dist_75", "dist_99", "dist_100",
    "octave_decoy_minus2", "octave_decoy_plus2", "partner_level_minus1", "partner_level_plus1",
    "u_at_maxu", "u_at_minu", "decoy_above_maxu", "decoy_below_minu",
    "band_o0_at_maxr", "band_o0_past_maxr", "band_o0_at_minr", "band_o0_before_minr",
    "band_top_at_maxr", "band_top_past_maxr", "band_top_at_minr", "band_top_before_minr",
    "clamp_row_0", "clamp_row_last", "fractional_vl", "no_candidate",
    "nr_zero", "nl_one", "nl_not_multiple_of_4", "nl_above_256",
    "inc_minus4", "inc_plus4", "inc_minus5", "inc_plus5", "equal_minimum_lower_offset",
    "endu_cols", "endu_cols_minus1", "zero_disparity", "negative_disparity", "disparity_at_maxd",
    "octave_gt0_default", "octave_gt0_pyr2", "octave_gt0_pyr15", "half_rounding",
    "median_one", "median_two", "median_odd", "median_even", "median_all_equal", "median_zero", "median_ties",
    "median_first_of_bucket", "median_last_of_bucket", "median_255", "median_256", "median_257",
    "cut_21_20", "cut_21_21", "cut_21_22", "cut_42_41", "cut_42_42", "cut_42_43", "cut_210_209", "cut_210_210",
    "cut_210_211", "sad_above_32768",
    *(f"median_{n}_{k}" for n in ("odd", "even", "ties", "first_of_bucket", "last_of_bucket", "255", "256", "257")
      for k in ("kept_below_th", "cut_at_th")), "accepted_index_above_256",
    "right_index_above_65535",
)


class _Builder:
    def __init__(self, name, seed, W=320, H=240, sf=1.2, nlevels=8, pads=(0, 0), block=1, noise=0, maxd=40.0):
        self.name, self.W, self.H = name, W, H
        self.rng = np.random.default_rng(seed)
        self.params = dict(nfeatures=500, scaleFactor=sf, nlevels=nlevels, iniThFAST=20, minThFAST=7)
        self.scale = np.ones(nlevels, f32)
        for l in range(1, nlevels):                       # ORBextractor.cc:419-424
            self.scale[l] = f32(self.scale[l - 1] * f32(sf))
        self.mb, self.mbf = 0.125, 0.125 * maxd           # maxD = mbf / mb exactly
        self.maxd = f32(maxd)
        tex = self.rng.integers(0, 256, ((H + block - 1) // block, (W + block - 1) // block), dtype=np.uint8)
        tex = np.kron(tex, np.ones((block, block), np.uint8))[:H, :W]
        if block > 1:   # a box filter of the block's size: a smooth texture whose coarse levels move with the image
            t = np.pad(tex.astype(np.float64), block // 2, mode="wrap")
            k = np.ones(block) / block
            t = np.apply_along_axis(np.convolve, 0, t, k, "same")
            t = np.apply_along_axis(np.convolve, 1, t, k, "same")
            tex = np.clip(np.rint((t[block // 2:block // 2 + H, block // 2:block // 2 + W] - 128) * 1.8 + 128), 0,
                          255).astype(np.uint8)
        # rows wider than the image where the case asks for an input row stride above the width
        self._lbuf = self.rng.integers(0, 256, (H, W + pads[0]), dtype=np.uint8)
        self._rbuf = self.rng.integers(0, 256, (H, W + pads[1]), dtype=np.uint8)
        self.left, self.right = self._lbuf[:, :W], self._rbuf[:, :W]
        self.left[:] = tex
        self.right[:, :W - SHIFT] = tex[:, SHIFT:]
        if noise:
            r = self.right.astype(np.int16) + self.rng.integers(-noise, noise + 1, self.right.shape)
            self.right[:] = np.clip(r, 0, 255).astype(np.uint8)
        self.kl, self.dl, self.kr, self.dr, self.plants = [], [], [], [], []

    # ---- keypoints and descriptors
    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flipped(self, q, d):
        bits = np.zeros(256, np.uint8)
        bits[self.rng.choice(256, d, replace=False)] = 1
        return q ^ np.packbits(bits)

    def L(self, x, y, octave=0, q=None):
        self.kl.append((f32(x), f32(y), 31.0 * float(self.scale[octave]), 0.0, 50.0, octave, -1))
        self.dl.append(self.desc() if q is None else q)
        return len(self.kl) - 1

    def R(self, x, y, octave=0, q=None):
        self.kr.append((f32(x), f32(y), 31.0 * float(self.scale[octave]), 0.0, 50.0, octave, -1))
        self.dr.append(self.desc() if q is None else q)
        return len(self.kr) - 1

    def at_level(self, xs, ys, octave):
        """The level-0 coordinates the extractor reports for level pixel (xs, ys) (ORBextractor.cc:1117-1121)."""
        return f32(f32(xs) * self.scale[octave]), f32(f32(ys) * self.scale[octave])

    def plant(self, item, iL, best_idx=None, best_dist=None, outcome=None, bestinc=None, sad=None, visible=False):
        self.plants.append(Plant(item, iL, best_idx, best_dist, outcome, bestinc, sad, visible))

    def pair(self, item, x, y, dist=10, octave=0, r_octave=None, r_xy=None, sad=None, q=None, **kw):
        """A left keypoint and its partner SHIFT pixels to the left (or at r_xy) at Hamming distance dist."""
        q = self.desc() if q is None else q
        iL = self.L(x, y, octave, q)
        rx, ry = (f32(x) - f32(SHIFT), y) if r_xy is None else r_xy
        iR = self.R(rx, ry, octave if r_octave is None else r_octave, self.flipped(q, dist))
        if sad is not None:
            self.plant_sad(int(round(float(rx))), int(round(float(y))), sad)
        if item:
            self.plant(item, iL, best_idx=iR, best_dist=dist, sad=sad, **kw)
        return iL, iR, q

    # ---- images
    def copy_site(self, cx, cy, d, hw=16):
        """The right image shows the left site around (cx, cy) at disparity d instead of SHIFT."""
        x0, x1 = max(cx - hw, d), min(cx + hw + 1, self.W)
        self.right[cy - 5:cy + 6, x0 - d:x1 - d] = self.left[cy - 5:cy + 6, x0:x1]

    def plant_sad(self, xr, y, v):
        """Raise the L1 distance of the right window centred (xr, y) to the identical left window by exactly v."""
        left = v
        for dy in (-5, -3, 3, 5, -4, 4):
            for dx in (-3, -1, 1, 3, -2, 2):
                if left == 0:
                    return
                p = int(self.right[y + dy, xr + dx])
                step = min(left, 100)
                self.right[y + dy, xr + dx] = p + step if p < 128 else p - step
                left -= step
        assert left == 0, "planted distance too large for plant_sad"

    def symmetric_site(self, cx, cy, hw=16):
        self.left[cy - 5:cy + 6, cx + 1:cx + hw + 1] = self.left[cy - 5:cy + 6, cx - hw:cx][:, ::-1]
        self.copy_site(cx, cy, SHIFT, hw)

    def band_edge(self, octave, y_row, edge):
        """A fractional right y at `octave` whose row band (Frame.cc:683-685) has `edge` ('maxr' / 'minr') == y_row."""
        r = f32(2.0) * self.scale[octave]
        for k in range(1, 400):
            yr = f32(y_row + (-1 if edge == "maxr" else 1) * (float(r) + 0.05 * k - 1.0))
            got = int(np.ceil(f32(yr + r))) if edge == "maxr" else int(np.floor(f32(yr - r)))
            if got == y_row and yr != np.floor(yr):
                return yr
        raise AssertionError("no y for the band edge")

    def done(self):
        kl = np.array(self.kl, KP_DTYPE) if self.kl else np.zeros(0, KP_DTYPE)
        kr = np.array(self.kr, KP_DTYPE) if self.kr else np.zeros(0, KP_DTYPE)
        dl = np.array(self.dl, np.uint8).reshape(-1, 32)
        dr = np.array(self.dr, np.uint8).reshape(-1, 32)
        for a in (self._lbuf, self._rbuf, kl, kr, dl, dr):
            a.setflags(write=False)
        return Case(self.name, self.left, self.right, kl, dl, kr, dr, self.mb, self.mbf, self.params,
                    tuple(self.plants))


def _ballast(b, rows, xs=(80, 160, 240), sad0=100):
    """Plain accepted octave-0 matches with planted window distances sad0, sad0 + 1, ...: they fix the median."""
    k = 0
    for cy in rows:
        for cx in xs:
            b.pair(None, cx, cy, dist=12, sad=sad0 + k)
            k += 1


def _search():
    """The descriptor search at octave 0 (default pyramid, maxD = 40)."""
    b = _Builder("search", 11)
    vis = dict(outcome=ACCEPTED, visible=True)
    rows = iter(range(24, 232, 16))
    # ties: lower iR wins; the decoy 14 px further left
    cy = next(rows)
    q = b.desc()
    iL = b.L(100, cy, 0, q)
    a = b.R(92, cy, 0, b.flipped(q, 20))
    b.R(78, cy, 0, b.flipped(q, 20))
    b.plant_sad(92, cy, 130)
    b.plant("tie_lower_ir", iL, best_idx=a, best_dist=20, sad=130, **vis)
    q = b.desc()
    iL = b.L(240, cy, 0, q)
    a = b.R(232, cy + 1, 0, b.flipped(q, 20))     # lower iR, later row
    b.R(218, cy - 1, 0, b.flipped(q, 20))
    b.plant_sad(232, cy, 131)
    b.plant("tie_lower_ir_later_row", iL, best_idx=a, best_dist=20, sad=131, **vis)
    # distances at the thresholds
    cy = next(rows)
    b.pair("dist_0", 100, cy, dist=0, sad=132, **vis)
    b.pair("dist_74", 240, cy, dist=74, sad=133, **vis)
    cy = next(rows)
    b.pair("dist_75", 100, cy, dist=75, outcome=DIST_HIGH)
    b.pair("dist_99", 240, cy, dist=99, outcome=DIST_HIGH)
    cy = next(rows)
    iL, _, _ = b.pair(None, 100, cy, dist=100)
    b.plant("dist_100", iL, best_idx=-1, best_dist=100, outcome=DIST_HIGH)
    # u range: partners exactly at maxU (disparity 0) and minU (disparity 40), decoys one ulp outside
    cy = next(rows)
    b.symmetric_site(100, cy)
    b.copy_site(100, cy, 0)
    b.pair("u_at_maxu", 100, cy, dist=10, r_xy=(f32(100), cy), outcome=CLAMPED, visible=True)
    q = b.desc()
    b.copy_site(240, cy, 20)
    iL, iR, _ = b.pair(None, 240, cy, dist=10, q=q, r_xy=(f32(220), cy))
    b.plant_sad(220, cy, 134)
    b.R(np.nextafter(f32(240), f32(1e9)), cy, 0, q)
    b.plant("decoy_above_maxu", iL, best_idx=iR, best_dist=10, sad=134, **vis)
    cy = next(rows)
    b.copy_site(100, cy, 40)
    uL = f32(99.75)                                   # minU = 59.75 rounds to column 60; disparity stays below 40
    b.pair("u_at_minu", uL, cy, dist=10, r_xy=(f32(uL - b.maxd), cy), **vis)
    b.plant_sad(60, cy, 135)
    q = b.desc()
    iL, iR, _ = b.pair(None, 240, cy, dist=10, sad=136, q=q)
    b.R(np.nextafter(f32(200), f32(-1e9)), cy, 0, q)
    b.plant("decoy_below_minu", iL, best_idx=iR, best_dist=10, sad=136, **vis)
    # row band of octave-0 right keypoints with fractional y 
    for cy, edge, inside in ((184, "maxr", True), (200, "maxr", False), (216, "minr", True), (184, "minr", False)):
        cx = 100 if inside or edge == "maxr" else 240
        name = "band_o0_" + {("maxr", True): "at_maxr", ("maxr", False): "past_maxr", ("minr", True): "at_minr",
                             ("minr", False): "before_minr"}[(edge, inside)]
        if inside:
            b.pair(name, cx, cy, dist=10, r_xy=(f32(cx - SHIFT), b.band_edge(0, cy, edge)), **vis)
            b.plant_sad(cx - SHIFT, cy, 137)
        else:
            q = b.desc()
            iL, iR, _ = b.pair(None, cx, cy, dist=10, sad=138, q=q)
            b.R(cx - SHIFT - 14, b.band_edge(0, cy - 1 if edge == "maxr" else cy + 1, edge), 0, q)
            b.plant(name, iL, best_idx=iR, best_dist=10, sad=138, **vis)
    # rows next to the image border (both clamps of the bucket lookup), a fractional vL, an empty row
    b.pair("clamp_row_0", 100, 5, dist=10, sad=139, **vis)
    b.pair("clamp_row_last", 100, 234, dist=10, sad=140, **vis)
    iL, _, _ = b.pair(None, 240, f32(10.6), dist=10, r_xy=(f32(232), f32(8.0)))   # band row 10, window row 11
    b.plant_sad(232, 11, 141)
    b.plant("fractional_vl", iL, best_idx=len(b.kr) - 1, best_dist=10, sad=141, **vis)
    iL = b.L(300, 150, 0)
    b.plant("no_candidate", iL, best_idx=-1, best_dist=100, outcome=NO_CANDIDATE)
    assert len(b.kl) % 4 != 0
    b.plant("nl_not_multiple_of_4", 0)
    return b.done()


def _octaves():
    """The octave gate around left keypoints at octave 2, on a smooth texture whose coarse levels still match: partners
    at octaves 1 and 3, distance-0 decoys at 0 and 4, 32 px (22 scaled pixels) from the partner.  The plain octave-2
    matches around them set the median, so the two partners survive the cut and mvuRight shows which keypoint won."""
    b = _Builder("octaves", 18, block=4, noise=2, maxd=80.0)
    sites = [(xs, ys) for ys in range(20, 150, 15) for xs in (70, 140, 200)]
    gate = (("partner_level_minus1", "octave_decoy_minus2", 1, 0), ("partner_level_plus1", "octave_decoy_plus2", 3, 4))
    for k, (xs, ys) in enumerate(sites):
        x, y = b.at_level(xs, ys, 2)
        if k in (4, 13):
            item_p, item_d, ro, do = gate[k == 13]
            q = b.desc()
            iL, iR, _ = b.pair(None, x, y, dist=10, octave=2, r_octave=ro, q=q)
            b.R(f32(x - 32), y, do, q)
            b.plant(item_p, iL, best_idx=iR, best_dist=10, outcome=ACCEPTED, visible=True)
            b.plant(item_d, iL, best_idx=iR, best_dist=10, outcome=ACCEPTED, visible=True)
        else:
            b.pair(None, x, y, octave=2)
    return b.done()


def _window():
    """The window search at octave 0."""
    b = _Builder("window", 12)
    rows = iter(range(24, 232, 16))
    cy = next(rows)
    for item, cx, k, out in (("inc_minus4", 100, 4, ACCEPTED), ("inc_plus4", 240, -4, ACCEPTED)):
        b.pair(item, cx, cy, r_xy=(f32(cx - SHIFT + k), cy), outcome=out, bestinc=-k, visible=True)
        b.plant_sad(cx - SHIFT, cy, 150 + k)
    cy = next(rows)
    for item, cx, k in (("inc_minus5", 100, 5), ("inc_plus5", 240, -5)):
        b.pair(item, cx, cy, r_xy=(f32(cx - SHIFT + k), cy), outcome=BEST_AT_L, bestinc=-k)
        b.plant_sad(cx - SHIFT, cy, 160 + k)
    cy = next(rows)                                   # texture of horizontal period 3: minima at -3, 0 and +3
    tile = np.tile(b.rng.integers(0, 256, (11, 3), dtype=np.uint8), (1, 16))
    b.left[cy - 5:cy + 6, 76:124] = tile
    b.right[cy - 5:cy + 6, 76 - SHIFT:124 - SHIFT] = tile
    b.pair("equal_minimum_lower_offset", 100, cy, outcome=ACCEPTED, bestinc=-3, sad=0, visible=True)
    cy = next(rows)                                   # the right window's last column against the level's last column
    b.copy_site(b.W - 8, cy, 4)
    b.pair("endu_cols_minus1", b.W - 8, cy, r_xy=(f32(b.W - 12), cy), outcome=ACCEPTED, visible=True)
    b.plant_sad(b.W - 12, cy, 170)
    cy = next(rows)
    b.copy_site(b.W - 7, cy, 4)
    b.pair("endu_cols", b.W - 7, cy, r_xy=(f32(b.W - 11), cy), outcome=WINDOW_OFF)
    cy = next(rows)                                   # symmetric sites at disparity 0: deltaR is exactly 0
    b.symmetric_site(100, cy)
    b.copy_site(100, cy, 0)
    b.pair("zero_disparity", 100, cy, r_xy=(f32(100), cy), outcome=CLAMPED, bestinc=0, sad=0, visible=True)
    b.symmetric_site(240, cy)
    b.copy_site(240, cy, 0)
    b.pair("negative_disparity", f32(239.7), cy, r_xy=(f32(239.6), cy), outcome=DISPARITY_RANGE, bestinc=0, sad=None)
    cy = next(rows)                                   # a symmetric site at disparity maxD: 40 < 40 fails
    b.symmetric_site(100, cy)
    b.copy_site(100, cy, 40)
    b.pair("disparity_at_maxd", 100, cy, r_xy=(f32(60), cy), outcome=DISPARITY_RANGE, bestinc=0, sad=0)
    _ballast(b, list(rows)[:3], sad0=140)
    return b.done()


def _levels(name, seed, item, **kw):
    """Left keypoints above octave 0 and the row band of top-octave right keypoints (maxD = 80)."""
    b = _Builder(name, seed, block=4, noise=2, maxd=80.0, **kw)
    top = b.params["nlevels"] - 1
    lo = top - 1                                      # the left keypoints' octave: windows on level top - 1
    s = float(b.scale[lo])
    cols, rows_ = int(b.W / s), int(b.H / s)
    far = int(np.ceil(14 * s))                        # decoy distance: 14 scaled pixels
    xs_all = [x for x in range(int((SHIFT + far) / s) + 12, cols - 7, int(90 / s) + 2)]
    edge = int(np.ceil((4 * float(b.scale[top]) + 3) / s))     # a band of the top octave two radii away stays inside
    ys_all = [y for y in range(max(8, edge), rows_ - max(8, edge), int(3 * float(b.scale[top]) / s) + 4)]
    sites = [(x, y) for y in ys_all for x in xs_all]
    assert len(sites) >= 8, (name, len(sites))
    names = {("maxr", True): "band_top_at_maxr", ("maxr", False): "band_top_past_maxr",
             ("minr", True): "band_top_at_minr", ("minr", False): "band_top_before_minr"}
    k = 0
    for edge in ("maxr", "minr"):
        for inside in (True, False):
            x, y = b.at_level(*sites[k], lo)
            k += 1
            row = int(y)
            if inside:
                b.pair(names[(edge, inside)], x, y, octave=lo, r_octave=top,
                       r_xy=(f32(x - SHIFT), b.band_edge(top, row, edge)), visible=True)
            else:
                q = b.desc()
                iL, iR, _ = b.pair(None, x, y, octave=lo, r_octave=top, q=q)
                b.R(f32(x - SHIFT - far), b.band_edge(top, row - 1 if edge == "maxr" else row + 1, edge), top, q)
                b.plant(names[(edge, inside)], iL, best_idx=iR, best_dist=10, visible=True)
    for xs, ys in sites[k:]:                          # plain matches at octave top - 1
        x, y = b.at_level(xs, ys, lo)
        b.pair(item, x, y, octave=lo)           # (the cut may take some: the census asks for five accepted ones)
    if b.params["scaleFactor"] == 2.0:
        # odd level-0 coordinates at octave 1: uL * 0.5 and uR0 * 0.5 are exact halves and round away from zero
        for cy in (21, 41, 61):
            b.pair("half_rounding", 101, cy, octave=1, visible=True)
            b.pair("half_rounding", 203, cy, octave=1, visible=True)
    return b.done()


def _many():
    """More than 256 left keypoints sharing sites (exact ties everywhere) and a band of more than 64 candidates."""
    b = _Builder("many", 14)
    vis = dict(outcome=ACCEPTED, visible=True)
    cy = 24
    q = b.desc()
    iL = b.L(100, cy, 0, q)
    for j in range(66):
        b.R(60 + j % 5, cy, 0)
    a = b.R(92, cy, 0, b.flipped(q, 20))
    b.R(70, cy, 0, b.flipped(q, 20))
    b.plant_sad(92, cy, 120)
    b.plant("tie_beyond_64", iL, best_idx=a, best_dist=20, sad=120, **vis)
    k = 0
    for cy in range(40, 232, 16):
        for cx in (80, 160, 240, 310):
            b.plant_sad(cx - SHIFT, cy, 100 + k % 40)
            for _ in range(6):
                iL, iR, _q = b.pair(None, cx, cy, dist=5 + k % 60)
                if iL > 256 and k % 7 == 0:
                    b.plant("accepted_index_above_256", iL, best_idx=iR, sad=100 + k % 40, **vis)
            k += 1
    assert len(b.kl) > 256
    b.plant("nl_above_256", len(b.kl) - 1)
    return b.done()


def _small(name, item, nl, nr):
    b = _Builder(name, 15)
    for i in range(nl):
        iL, _, _ = b.pair(None, 100 + 70 * (i % 3), 40 + 16 * (i // 3), sad=100 + i)
    if nr == 0:
        b.kr, b.dr = [], []
        b.plant(item, 0, best_idx=-1, best_dist=100, outcome=NO_CANDIDATE)
    else:
        b.plant(item, 0, best_idx=0, best_dist=10, sad=100, outcome=ACCEPTED, visible=True)
    return b.done()


def _median(name, seed, sads, plants):
    """One call whose accepted window distances are exactly `sads` (octave 0); plants: (item, position, outcome)."""
    b = _Builder(name, seed)
    idx = []
    for i, v in enumerate(sads):
        iL, iR, _ = b.pair(None, 100 + 70 * (i % 3), 24 + 16 * (i // 3), sad=v)
        idx.append((iL, iR))
    for item, i, outcome in plants:
        b.plant(item, idx[i][0], best_idx=idx[i][1], best_dist=10, sad=sads[i], outcome=outcome, bestinc=0)
    return b.done()


def th_dist(median):
    """thDist of Frame.cc:824 in float32."""
    return f32(f32(f32(1.5) * f32(1.4)) * f32(median))


def _flip_case(name, seed, lows, p, m, extra=()):
    """A median case whose cut shows the selected median: sorted, the distances are lows + [p, m, a, b] + extra with
    the median m at position count / 2, p <= m the element before it, a the largest integer below thDist(m) and b = a + 1.
    The right median keeps a and cuts b.  The element before it (or any median up to p) cuts a as well; the element
    after it (a itself) keeps b.  The distances are planted in a scrambled order."""
    a = int(np.ceil(float(th_dist(m)))) - 1
    assert f32(a) < th_dist(m) <= f32(a + 1) and (p == m or f32(a) >= th_dist(p)) and p <= m
    sads = list(lows) + [p, m, a, a + 1] + list(extra)
    assert sorted(sads)[len(sads) // 2] == m and all(v <= p for v in lows) and all(v > a + 1 for v in extra)
    order = [(7 * i + 3) % len(sads) for i in range(len(sads))] if len(sads) % 7 else list(range(len(sads)))[::-1]
    assert sorted(order) == list(range(len(sads)))
    planted = [sads[j] for j in order]
    pos = {j: i for i, j in enumerate(order)}
    n = len(lows)
    return _median(name, seed, planted, [(name, pos[n + 1], ACCEPTED), (name + "_kept_below_th", pos[n + 2], ACCEPTED),
                                         (name + "_cut_at_th", pos[n + 3], CUT)])


def _huge_sad():
    """Window distances above 32768.  The left window is 255 around a centre of 0.  The right strip is 0 except its
    centre row (255): every offset then costs 10 * 255 + 110 * 510 = 58650, less 255 per white pixel planted in the
    window.  w white pixels go into each of the columns -5.. and +5.. of the strip (column 5 first), so offset 0 sees
    2w of them and every other offset fewer.  No distance can be 2.1 times another one above 32768 (121 * 510 is the
    most), so the cut keeps them all; a median that lost its high bits (below 58140 / 2.1) cuts the largest."""
    b = _Builder("median_above_32768", 40)
    for i, w in enumerate((1, 10, 25, 40, 50)):
        cx, cy = 100 + 70 * (i % 3), 24 + 16 * (i // 3)
        b.left[cy - 5:cy + 6, cx - 5:cx + 6] = 255
        b.left[cy, cx] = 0
        xr = cx - SHIFT
        b.right[cy - 5:cy + 6, xr - 12:xr + 13] = 0
        b.right[cy, xr - 12:xr + 13] = 255
        cells = [(dy, c) for c in (5, 4, 3, 2, 1) for dy in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)][:w]
        for dy, c in cells:
            b.right[cy + dy, xr - c] = 255
            b.right[cy + dy, xr + c] = 255
        sad = 58650 - 510 * w
        assert sad > 32768
        b.pair("sad_above_32768", cx, cy, sad=None, outcome=ACCEPTED, bestinc=0, visible=True)
        b.plants[-1] = b.plants[-1]._replace(sad=sad)
    return b.done()


def _big_nr():
    """More than 65,535 right keypoints: every partner's index is at least 65,536; the keypoint at that index modulo
    65,536 lies in another row at another x.  The filler sits in rows that no left keypoint's band reaches."""
    b = _Builder("big_nr", 50)
    for j in range(64):
        b.R(30 + 3 * j, 215, 0)
    n_fill = 65540 - 64
    xs = b.rng.integers(10, 300, n_fill + 54)
    zero = np.zeros(32, np.uint8)
    for j in range(n_fill):
        b.R(xs[j], 230, 0, zero)
    for i in range(6):
        iL, iR, _ = b.pair(None, 150 + 20 * (i % 2), 24 + 16 * i, sad=100 + i)
        assert iR >= 65536 and b.kr[iR & 0xFFFF][0] != b.kr[iR][0]
        b.plant("right_index_above_65535", iL, best_idx=iR, best_dist=10, sad=100 + i, outcome=ACCEPTED, visible=True)
    for j in range(54):
        b.R(xs[n_fill + j], 230, 0, zero)
    return b.done()


def _cut_case(m):
    v = {10: 21, 20: 42, 100: 210}[m]
    sads = [m] * 5 + [v - 1, v, v + 1]
    return _median(f"cut_{v}", 30 + m, sads, [(f"cut_{v}_{v - 1}", 5, None), (f"cut_{v}_{v}", 6, None),
                                              (f"cut_{v}_{v + 1}", 7, None)])


_BUILDERS = {
    "search": _search,
    "window": _window,
    "octaves": _octaves,
    # odd dimensions and input rows wider than the image, for both images
    "levels_odd_strided": lambda: _levels("levels_odd_strided", 13, "octave_gt0_default", W=323, H=241, pads=(29, 61)),
    # scaleFactor 2.0: exact halves under the inverse scale (a fourth level would need an image of 496 x 496 for
    # the extractor's cell grid, so the bucket lookup's reach is ceil(2 * 4) + 1 = 9 as for the default pyramid)
    "levels_pyr2": lambda: _levels("levels_pyr2", 16, "octave_gt0_pyr2", W=320, H=256, sf=2.0, nlevels=3),
    # scaleFactor 1.5, four levels: reach = ceil(2 * 3.375) + 1 = 8
    "levels_pyr15": lambda: _levels("levels_pyr15", 17, "octave_gt0_pyr15", sf=1.5, nlevels=4),
    "many": _many,
    "nr_zero": lambda: _small("nr_zero", "nr_zero", 5, 0),
    "nl_one": lambda: _small("nl_one", "nl_one", 1, 1),
    "median_one": lambda: _median("median_one", 20, [120], [("median_one", 0, ACCEPTED)]),
    "median_two": lambda: _median("median_two", 21, [100, 250], [("median_two", 1, ACCEPTED)]),   # 250 < 2.1 * 250 only
    "median_odd": lambda: _flip_case("median_odd", 22, [100], 110, 120),
    "median_even": lambda: _flip_case("median_even", 23, [90, 100], 110, 120),
    "median_all_equal": lambda: _median("median_all_equal", 24, [77] * 6, [("median_all_equal", 5, ACCEPTED)]),
    "median_zero": lambda: _median("median_zero", 25, [0, 9, 0, 5, 0], [("median_zero", 0, CUT)]),
    "median_ties": lambda: _flip_case("median_ties", 26, [50, 90, 90, 90], 90, 90),
    # sorted 10 10 10 20 20 41 42: element 3 is the first 20; the 10 before it would cut 41 as well
    "median_first_of_bucket": lambda: _median("median_first_of_bucket", 27, [20, 41, 10, 42, 10, 20, 10],
                                              [("median_first_of_bucket", 0, ACCEPTED),
                                               ("median_first_of_bucket_kept_below_th", 1, ACCEPTED),
                                               ("median_first_of_bucket_cut_at_th", 3, CUT)]),
    # sorted 10 10 20 20 41 42 60: element 3 is the last 20; the 41 after it would keep 42 and 60
    "median_last_of_bucket": lambda: _median("median_last_of_bucket", 28, [20, 42, 10, 60, 41, 10, 20],
                                             [("median_last_of_bucket", 0, ACCEPTED),
                                              ("median_last_of_bucket_kept_below_th", 4, ACCEPTED),
                                              ("median_last_of_bucket_cut_at_th", 1, CUT)]),
    "median_255": lambda: _flip_case("median_255", 29, [253], 254, 255),
    "median_256": lambda: _flip_case("median_256", 30, [253, 254], 255, 256),
    "median_257": lambda: _flip_case("median_257", 31, [255], 256, 257),
    "cut_21": lambda: _cut_case(10),
    "cut_42": lambda: _cut_case(20),
    "cut_210": lambda: _cut_case(100),
    "median_above_32768": _huge_sad,
    "big_nr": _big_nr,
}
CASES = tuple(_BUILDERS)
# what the median of a median_* / cut_* case must be (the census checks the reference trace against it)
MEDIANS = {"median_one": 120, "median_two": 250, "median_odd": 120, "median_even": 120, "median_all_equal": 77,
           "median_zero": 0, "median_ties": 90, "median_first_of_bucket": 20, "median_last_of_bucket": 20,
           "median_255": 255, "median_256": 256, "median_257": 257, "cut_21": 10, "cut_42": 20, "cut_210": 100}


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def oracle_pair(oracle_mod, c):
    """The two oracle extractors after running on the case's image pair."""
    p = c.params
    ol, orr = (oracle_mod.OracleExtractor(p["nfeatures"], p["scaleFactor"], p["nlevels"], p["iniThFAST"],
                                          p["minThFAST"]) for _ in range(2))
    assert ol.run(c.left) >= 0 and orr.run(c.right) >= 0
    return ol, orr


_expected = {}


def expected(oracle_mod, name):
    """(uright, depth, nmatched, trace, levels_l) of tests/stereo_ref.py on a case, computed once and left unchanged."""
    if name not in _expected:
        import stereo_ref
        c = case(name)
        ol, orr = oracle_pair(oracle_mod, c)
        t = ol.tables()
        ll = [ol.level(l) for l in range(c.params["nlevels"])]
        lr = [orr.level(l) for l in range(c.params["nlevels"])]
        u, d, n, trace = stereo_ref.compute_stereo_matches(ll, lr, t["scale"], t["inv_scale"], c.kl, c.dl, c.kr, c.dr,
                                                           c.mb, c.mbf)
        u.setflags(write=False)
        d.setflags(write=False)
        _expected[name] = (u, d, n, trace, ll, lr, t)
    return _expected[name]
