"""Planted inputs for the cell staging of k_fast_wave / flow_fast (csrc/extract_kernels.hip), pure numpy.

Part 1 restates build_cells / fast_cell_t / fast_wave_layout for a (width, height, levels): per level the cell size,
per cell the quantities the staging code branches on, per context the tile pitch.  Part 2 plants decisions on a flat
background, one group per cell, where the staging could go wrong: how the ROI reaches the 16-bit LDS tile (aligned
dwords widened in registers for the ROI's byte offset B in its first dword, or byte by byte), at which pitch, and
how the prefilter's lanes (16-pixel runs, row rounds of rpi rows) and the late-loaded rows of a tall ROI map onto it.

Tile geometry: ROI column c is tile element c + 1; domain pixel (x, y) is ROI (x + 3, y + 3).  A prefilter lane
takes the 16 pixels [16 r, 16 r + 16) of a domain row as two windows of 8 (prefilter16); the compass pixels at
columns -3 / +3 come from the same row's neighbouring dwords, so for a centre at x = 16 r + 7 or 16 r + 15 column
+3 belongs to the next window / run and for x = 16 r + 8 or 16 r column -3 belongs to the previous one.

The sizes (level 0 unless noted; every frame has its smallest level count):

    180 x 91, 1 level   4 x 1 cells, wCell 37, hCell 59 (ROI 43 x 59, domain 37 x 53; the last cell 31 wide): B = 0, 1,
                        2, 3, three runs, rpi = 21 (three row rounds, the last of 11 rows), nw = 11 or 12, rpr = 5,
                        ROI rows 40..58 loaded late; pitch 80; stride 180
    179 x 91, 1 level   the same grid (last cell 30 wide) at an odd stride: BatchExtractor stores it byte by byte
    108 x 91, 1 level   two cells, ROI 44 and 38 wide at B = 0 and B = 2: B + rw is a multiple of 4, so the ROI's
                        last column is byte 3 of the row's last dword, the even form's third store (b3, 0)
    91 x 91,  1 level   one cell, ROI 59 x 59, domain 53 x 53 (the largest a grid gives): four runs, rpi = 16, four
                        rounds (the last of 5 rows), nw = 15, rpr = 4; an odd stride for BatchExtractor, aligned
                        through ORBextractor's operator()
    364 x 101, 2 levels pitch 48: level 0 is 11 x 2 cells of 31 x 35 / 31 x 28 (B = 0, 3, 2, 1, ...; 3 tail rows in
                        grid row 0; the last column 16 wide at B = 2 with the third store); level 1 (303 x 84) is one
                        row of cells with ROI 37 x 52 (rh > 8 * rpr = 48: late rows at pitch 48)

Every size has NROT planted frames and one of noise.  Planted frame r gives cell (ci, cj) of level 0 the group
GROUPS[(2 ci + cj + r) mod 5], so every cell (every B, every shape) holds every group once:

    dots     single pixels (arc strength |v - BG|): the domain's four corner pixels, the last row of each row round
             and the first of the next, the last prefetched ROI row (8 rpr - 1) and the first late-loaded one
    seamA/B  9-arcs of strength iniTh + 1, each 7 rows above a twin of exactly iniTh (no corner), centred at
             x = 7, 8, 15, 16, 31, 32, 47, 48 and dw - 1, dw - 2, dw - 4.  The arc holds two compass pixels, one of
             each pair (p0 | p8), (p4 | p12): p4 (column +3) for a centre left of a seam, p12 (column -3) right of it,
             so the decision rests on a pixel the lane reads from the next / previous window, run, or past the domain
    weak     nothing at iniTh; dots of minTh + 1 in two row rounds, in a late-loaded row and at the last pixel, and
             dots of exactly minTh: the second pass runs over every round
    plateau  two pairs of adjacent equal dots (corners at iniTh that the NMS drops, in two row rounds) and one dot of
             minTh + 2: pass 0 keeps nothing, its map entries are cleared, pass 1 keeps the weak corner

A Plant's carrier names the compass pixel ("p4", "p12") on the far side of the seam, or is None for dots."""
import math

import numpy as np

from test_fast_arc_planted import CIRCLE, _arc, _plant, _strength   # noqa: F401  (the arc helpers, as they are)
from test_gpu_fast_tail import BORDER, _level_sizes, _noise          # noqa: F401

BG, INI_TH, MIN_TH, NFEAT = 100, 20, 7, 500
PITCH_COMPACT, PITCH_WIDE = 48, 80        # fast_wave_layout: 48 elements if every level's wCell <= 36, else 80
PX = 16                                    # pixels of a prefilter run


# ----------------------------------------------------------------------------------------------------------------
# Part 1: the geometry model
# ----------------------------------------------------------------------------------------------------------------
class Cell:
    """One valid cell, as build_cells / fast_cell_t derive it."""

    def __init__(self, level, ci, cj, ini_x, ini_y, rw, rh):
        self.level, self.ci, self.cj, self.ini_x, self.ini_y, self.rw, self.rh = level, ci, cj, ini_x, ini_y, rw, rh
        self.dw, self.dh = rw - 6, rh - 6
        self.B = ini_x & 3                                   # the ROI's byte offset in its first dword
        x0w = ini_x >> 2
        self.nw = max(1, ((ini_x + rw + 3) >> 2) - x0w)      # dwords per ROI row
        self.rpr = 64 // self.nw                             # ROI rows per load round
        self.late = rh > 8 * self.rpr                        # rows 8 rpr.. are loaded in widen_rows' last loop
        self.nruns = max(1, (self.dw + 15) // 16)
        self.rpi = 64 // self.nruns                          # domain rows per prefilter round
        self.np = max(1, (self.dw + 1) // 2)
        trows = self.dh % self.rpi
        self.tail = trows if trows * self.np <= 64 else 0    # (run as pixel pairs only at the compact pitch)
        self.rounds = -(-self.dh // self.rpi)                # row rounds without the tail form
        self.partial = self.dh % self.rpi                    # rows of the last round if it is not full
        # the even form's extra store (b3, 0) of a row's last dword carries ROI column rw - 1 iff B + rw is a
        # multiple of 4; otherwise it holds a byte past the ROI
        self.last_b3 = self.B % 2 == 0 and (self.B + rw) % 4 == 0

    def origin(self):
        """Image coordinates of domain pixel (0, 0)."""
        return self.ini_x + 3, self.ini_y + 3

    def where(self, ox, oy):
        """(row round, run, late-loaded ROI row?) of domain pixel (ox, oy)."""
        return oy // self.rpi, ox // PX, oy + 3 >= 8 * self.rpr

    def tag(self, pitch):
        return "pitch %d L%d cell (%d, %d) %dx%d B=%d nw=%d rpr=%d nruns=%d rpi=%d tail=%d late=%s" % (
            pitch, self.level, self.ci, self.cj, self.dw, self.dh, self.B, self.nw, self.rpr, self.nruns, self.rpi,
            self.tail if pitch == PITCH_COMPACT else 0, self.late)


class Level:
    def __init__(self, level, w, h):
        self.level, self.w, self.h = level, w, h
        max_bx, max_by = w - BORDER, h - BORDER
        width, height = np.float32(max_bx - BORDER), np.float32(max_by - BORDER)
        self.ncols, self.nrows = int(width / np.float32(30)), int(height / np.float32(30))
        self.wcell, self.hcell = int(math.ceil(width / self.ncols)), int(math.ceil(height / self.nrows))
        self.cells = []
        for ci in range(self.nrows):
            for cj in range(self.ncols):
                ini_y, ini_x = BORDER + ci * self.hcell, BORDER + cj * self.wcell
                if ini_y >= max_by - 3 or ini_x >= max_bx - 6:
                    continue
                rw = min(ini_x + self.wcell + 6, max_bx) - ini_x
                rh = min(ini_y + self.hcell + 6, max_by) - ini_y
                if rw - 6 <= 0 or rh - 6 <= 0:
                    continue
                self.cells.append(Cell(level, ci, cj, ini_x, ini_y, rw, rh))

    def cell(self, ci, cj):
        return next(c for c in self.cells if (c.ci, c.cj) == (ci, cj))


class Geometry:
    """The cells of every level of a w x h frame and the context's tile pitch."""

    def __init__(self, w, h, nlevels):
        self.w, self.h, self.nlevels = w, h, nlevels
        self.levels = [Level(l, lw, lh) for l, (lw, lh) in enumerate(_level_sizes(w, h, nlevels))]
        self.pitch = PITCH_COMPACT if max(L.wcell for L in self.levels) <= 36 else PITCH_WIDE

    def cells(self):
        return [c for L in self.levels for c in L.cells]

    def level0_aligned(self, row_stride):
        """fast_cell_t: a level is loaded as dwords iff its base and row stride are multiples of 4.  Frames come
        from the allocator (base aligned); the pyramid's levels have 64-byte rows."""
        return row_stride % 4 == 0


# name -> (width, height, levels)
SIZES = {"w180": (180, 91, 1), "w179": (179, 91, 1), "w108": (108, 91, 1), "w91": (91, 91, 1), "w364": (364, 101, 2)}
# the BASELINE configurations' frame sizes, all at 8 levels
BENCH_SIZES = {"C1": (640, 480), "C2": (640, 480), "C3": (1280, 720), "C4": (1280, 720), "C5": (1280, 720)}


# ----------------------------------------------------------------------------------------------------------------
# Part 2: the planted frames
# ----------------------------------------------------------------------------------------------------------------
class Plant:
    """One planted decision.  (ox, oy): domain pixel in its cell; m: designed arc strength; kept: a candidate of the
    planted level; carrier: the compass pixel on the far side of the seam that alone carries the prefilter's
    decision (None for dots); want: what the position was chosen for, checked against the model by
    tests/test_fast_stage_cases.py ({"round": k}, {"run": r}, {"late": bool})."""

    def __init__(self, group, name, cell, ox, oy, m, kept, carrier=None, want=None):
        self.group, self.name, self.cell, self.ox, self.oy, self.m, self.kept = group, name, cell, ox, oy, m, kept
        self.carrier, self.want = carrier, dict(want or {})
        x0, y0 = cell.origin()
        self.x, self.y = x0 + ox, y0 + oy

    def __repr__(self):
        return "%s/%s at (%d, %d) = cell (%d, %d) + (%d, %d) M=%d %s%s" % (
            self.group, self.name, self.x, self.y, self.cell.ci, self.cell.cj, self.ox, self.oy, self.m,
            "kept" if self.kept else "not kept", " carrier " + self.carrier if self.carrier else "")


# the order places the groups' neighbours: the circle of seamA's centre at x = dw - 1 reaches three columns into the
# cell on its right, which is seamB's (its centres start at x = 7), never a weak or plateau cell (an arc pixel
# differs from the background by more than minTh and would be a corner of the second pass)
GROUPS = ["dots", "weak", "plateau", "seamA", "seamB"]
# 9-arc starts whose arc holds exactly two compass pixels: p4 with p8 / p0 (column +3 carries), p12 with p8 / p0
P4_STARTS, P12_STARTS = [1, 15, 3, 13, 2, 14, 1], [5, 11, 7, 9]


def _seam_wanted(c):
    """Seam centres of a cell: (x, carrier, seam) in placement priority; x + 3 / x - 3 lies across the named seam."""
    out = [(c.dw - 1, "p4", "domain"), (c.dw - 2, "p4", "domain"), (c.dw - 4, "p4", "domain")]
    for x in (7, 15, 31, 47):
        if x + 3 < c.dw and x < c.dw - 4:
            out.append((x, "p4", "run" if x % 16 == 15 else "window"))
    for x in (8, 16, 32, 48):
        if x < c.dw:
            out.append((x, "p12", "run" if x % 16 == 0 else "window"))
    return out


def _seam_bins(c, last_row):
    """Greedy packing of the seam centres into row pairs (plant at y, twin at y + 7; centres of a row >= 7 apart):
    the pairs of seamA first, then seamB's.  A twin may sit in the domain's last rows only if no cell lies below."""
    ymax = c.dh - 1 if last_row else c.dh - 4
    pairs = [6 + 14 * k for k in range(8) if 13 + 14 * k <= ymax]
    bins = [(g, y, []) for g in ("seamA", "seamB") for y in pairs]
    for w in _seam_wanted(c):
        for g, y, xs in bins:
            if all(abs(w[0] - o[0]) >= 7 for o in xs):
                xs.append(w)
                break
        else:
            raise AssertionError(("no room for seam centre", w, c.dw, c.dh))
    return bins


def _group_plants(group, c, last_row):
    """The plants of `group` in cell c, and [(x, y, value)] pixels / [(x, y, v, ring)] patterns in domain coordinates."""
    plants, dots, arcs = [], [], []

    def dot(name, ox, oy, d, kept, **want):
        if 0 <= ox < c.dw and 0 <= oy < c.dh:
            dots.append((ox, oy, BG + d))
            plants.append(Plant(group, name, c, ox, oy, abs(d), kept, None, want))

    if group == "dots":
        dot("first pixel", 0, 0, 31, True, round=0, run=0)
        dot("last pixel of row 0", c.dw - 1, 0, -33, True, round=0, run=c.nruns - 1)
        dot("first pixel of the last row", 0, c.dh - 1, 35, True, round=c.rounds - 1, run=0)
        dot("last pixel", c.dw - 1, c.dh - 1, -37, True, round=c.rounds - 1, run=c.nruns - 1)
        for k in range(1, c.rounds):      # the last row of round k - 1 and the first of round k
            xa = 6 if k % 2 else min(20, c.dw - 10)
            dot("last row of round %d" % (k - 1), xa, k * c.rpi - 1, 40 + k, True, round=k - 1)
            dot("first row of round %d" % k, xa + 5, k * c.rpi, -(50 + k), True, round=k)
        if c.late:                        # ROI rows 8 rpr - 1 (the last prefetched) and 8 rpr (the first loaded late)
            dot("last prefetched row", c.dw - 8, 8 * c.rpr - 4, 60, True, late=False)
            dot("first late row", max(c.dw - 14, 1), 8 * c.rpr - 3, -62, True, late=True)
    elif group in ("seamA", "seamB"):
        n4 = n12 = 0
        for g, y, xs in _seam_bins(c, last_row):
            if g != group:
                continue
            for x, carrier, seam in xs:
                if carrier == "p4":
                    first, bright, n4 = P4_STARTS[n4 % len(P4_STARTS)], n4 % 2 == 0, n4 + 1
                else:
                    first, bright, n12 = P12_STARTS[n12 % len(P12_STARTS)], n12 % 2 == 0, n12 + 1
                # bright: centre BG - 11 under an arc of BG + 10 (M = 21); dark: centre BG + 11 over BG - 10.  No
                # pixel differs from the background by more than iniTh: the centre is the pattern's only corner
                v, a = (BG - 11, BG + 10) if bright else (BG + 11, BG - 10)
                name = "%s seam at x = %d, %s arc from %d" % (seam, x, "bright" if bright else "dark", first)
                arcs.append((x, y, v, _arc(first, a)))
                plants.append(Plant(group, name, c, x, y, INI_TH + 1, True, carrier, {"run": x // PX, "seam": seam}))
                arcs.append((x, y + 7, v + (1 if bright else -1), _arc(first, a)))
                plants.append(Plant(group, name + ", twin at iniTh", c, x, y + 7, INI_TH, False, carrier,
                                    {"run": x // PX, "seam": seam}))
    elif group == "weak":   # nothing at iniTh: the minTh pass runs over every row round
        dot("weak, round 0", 5, 2, MIN_TH + 1, True, round=0)
        if c.rounds > 1:
            dot("weak, round 1", c.dw - 9, c.rpi + 1, -(MIN_TH + 1), True, round=1)
        if c.late:
            dot("weak, late row", 9, min(8 * c.rpr + 2, c.dh - 2), MIN_TH + 1, True, late=True)
        dot("weak, last pixel", c.dw - 1, c.dh - 1, 15, True, round=c.rounds - 1, run=c.nruns - 1)
        dot("exactly minTh", 14, c.rpi - 1 if c.rounds > 1 else 9, MIN_TH, False)
        dot("exactly -minTh", 20, 6, -MIN_TH, False)
    elif group == "plateau":   # pass 0 finds the pairs and keeps none; pass 1 keeps the weak corner
        dot("equal pair, left", 6, 3, 40, False, round=0)
        dot("equal pair, right", 7, 3, 40, False, round=0)
        y1 = c.rpi + 2 if c.rounds > 1 and c.rpi + 3 < c.dh - 4 else 12
        dot("equal dark pair, upper", 12, y1, -45, False, round=y1 // c.rpi)
        dot("equal dark pair, lower", 12, y1 + 1, -45, False, round=(y1 + 1) // c.rpi)
        dot("weak corner after the plateau", c.dw - 6, c.dh - 2, MIN_TH + 2, True, round=c.rounds - 1)
    return plants, dots, arcs


def build_frame(geo, rot):
    """Planted frame `rot` of a geometry: cell (ci, cj) of level 0 holds group (ci * 2 + cj + rot) mod 5.
    Returns (image, [Plant], {(ci, cj): group})."""
    L0 = geo.levels[0]
    img = np.full((geo.h, geo.w), BG, np.uint8)
    plants, groups = [], {}
    for c in L0.cells:
        group = GROUPS[(c.ci * 2 + c.cj + rot) % len(GROUPS)]
        groups[(c.ci, c.cj)] = group
        ps, dots, arcs = _group_plants(group, c, c.ci == L0.nrows - 1)
        x0, y0 = c.origin()
        for ox, oy, v in dots:
            img[y0 + oy, x0 + ox] = v
        for ox, oy, v, ring in arcs:
            _plant(img, x0 + ox, y0 + oy, v, ring)
        plants += ps
    # no plant on another's circle or beside it: dots >= 4 px apart in x or y, patterns >= 7, a dot clear of a pattern
    for i, p in enumerate(plants):
        for q in plants[:i]:
            need = 4 if p.carrier is None and q.carrier is None else 7 if p.carrier and q.carrier else 5
            adjacent_pair = p.group == q.group == "plateau" and abs(p.x - q.x) + abs(p.y - q.y) == 1
            assert adjacent_pair or max(abs(p.x - q.x), abs(p.y - q.y)) >= need, ("plants too close", p, q)
    return img, plants, groups


NROT = len(GROUPS)


def frames(name):
    """The frames of a size: NROT planted frames (every cell holds every group once) and one of noise."""
    w, h, nlevels = SIZES[name]
    geo = Geometry(w, h, nlevels)
    planted = [build_frame(geo, r) for r in range(NROT)]
    return geo, planted, np.stack([p[0] for p in planted] + [_noise(w, h, 11)])


_EXPECTED = {}


def expected(oracle_mod, name):
    """(geometry, planted frames, all frames, per frame the oracle's (candidates per level, keypoints, descriptors)),
    computed once per size and shared by the CPU and the GPU tests."""
    if name not in _EXPECTED:
        geo, planted, fr = frames(name)
        per = []
        for img in fr:
            o = oracle_mod.OracleExtractor(NFEAT, 1.2, geo.nlevels, INI_TH, MIN_TH)
            kps, desc = o(img)
            per.append(([o.candidates(l).copy() for l in range(geo.nlevels)], kps.copy(), desc.copy()))
        _EXPECTED[name] = (geo, planted, fr, per)
    return _EXPECTED[name]


def explain(geo, planted, frame, level, got, want):
    """Names the cells (with the staging tuple of each) and the plants where two candidate lists differ."""
    g = {(int(x), int(y)): int(r) for x, y, r in got}
    w = {(int(x), int(y)): int(r) for x, y, r in want}
    lines = []
    for key in sorted(set(g) | set(w), key=lambda k: (k[1], k[0])):
        if g.get(key) == w.get(key):
            continue
        x, y = key[0] + BORDER, key[1] + BORDER
        c = cell_of(geo, x, y, level)
        plant = None
        if level == 0 and frame < len(planted):
            plant = next((p for p in planted[frame][1] if (p.x, p.y) == (x, y)), None)
        where = ""
        if c is not None:
            x0, y0 = c.origin()
            where = "%s; pixel (%d, %d) round %d run %d late row %s" % ((c.tag(geo.pitch), x - x0, y - y0) +
                                                                          c.where(x - x0, y - y0))
        lines.append("(%d, %d): got %s, oracle %s; %s; %s" % (x, y, g.get(key), w.get(key), where,
                                                             plant if plant else "no plant"))
        if len(lines) == 6:
            break
    return lines


def cell_of(geo, x, y, level=0):
    """The cell of level `level` whose domain holds image pixel (x, y), or None."""
    for c in geo.levels[level].cells:
        x0, y0 = c.origin()
        if x0 <= x < x0 + c.dw and y0 <= y < y0 + c.dh:
            return c
    return None
