"""Planted inputs for k_octree (csrc/extract_kernels.hip: octree_task / octree_level), pure numpy.

Every frame is a flat background with *stamps*: one pixel brighter than the background by d is a FAST corner of
response d - 1 that none of its neighbours sees as a corner; stamps are at least 4 px apart (in x or in y), so none
lies on another's ring.  The extractors have one level (nlevels = 1), so N == nfeatures and the candidates are the
stamps and nothing else.  Two frame sizes (cell sizes from ORBextractor.cc:781-790):

    320 x 240: border-trimmed 288 x 208, 9 x 6 cells of 32 x 35, nIni = 1, hX = 288
    640 x 240: border-trimmed 608 x 208, 20 x 6 cells of 31 x 35, nIni = 3, hX = 202.67 (roots start at 0, 202, 405)

A case is a frame and an N; one frame serves several N.  The depth F of the kernel's fast-forward tables (ff_depth:
the first depth d <= 6 with nIni * 4^d >= N, when the tables fit the node area) for the N used here:

    nIni = 1:  N <= 4: F = 1;  5..16: F = 2;  17..64: F = 3;  65..256: F = 4;  257..1024: F = 5;  above: F = 6
    nIni = 3:  N <= 12: F = 1;  13..48: F = 2;  49..192: F = 3;  193..768: F = 4

census(case, tr0, out0, out1, cands) names the census items a case realises, from the trace of tests/octree_ref.py
alone plus the launch facts restated here (node_cap, ff_depth, the sort path and its waves, the LDS key room of the
single-frame and of the dataflow launch); tests/test_octree_cases.py asserts that every item of CENSUS is realised by a case that claims it."""
import numpy as np

BORDER = 16          # EDGE_THRESHOLD - 3: candidates are relative to it
H = 240
BG = 0
INI_TH, MIN_TH = 20, 7


class Geo:
    def __init__(self, w):
        self.w, self.h = w, H
        self.width, self.height = w - 2 * BORDER, H - 2 * BORDER            # maxBorder - minBorder
        self.ncols, self.nrows = self.width // 30, self.height // 30        # :781-784
        self.wcell = -(-self.width // self.ncols)
        self.hcell = -(-self.height // self.nrows)
        self.nini = int(round(self.width / self.height))

    def cell(self, x, y):
        return (y - 3) // self.hcell, (x - 3) // self.wcell

    def inside(self, x, y):
        return 3 <= x < self.width - 3 and 3 <= y < self.height - 3


G320, G640 = Geo(320), Geo(640)


class Frame:
    """Stamps as {(x, y): response}, coordinates relative to the border."""

    def __init__(self, name, geo, stamps):
        self.name, self.geo = name, geo
        pts = sorted(stamps)
        for x, y in pts:
            assert geo.inside(x, y), (name, x, y)
            assert 20 <= stamps[(x, y)] <= 254, (name, x, y)
        occ = np.zeros((geo.height + 8, geo.width + 8), bool)
        for x, y in pts:      # at least 4 px apart: no other stamp in the 7 x 7 around one
            assert not occ[y + 4 - 3:y + 4 + 4, x + 4 - 3:x + 4 + 4].any(), (name, "stamps closer than 4 px", x, y)
            occ[y + 4, x + 4] = True
        self.stamps = dict(stamps)

    def image(self):
        img = np.full((self.geo.h, self.geo.w), BG, np.uint8)
        for (x, y), r in self.stamps.items():
            img[y + BORDER, x + BORDER] = BG + r + 1
        return img

    def candidates(self):
        """The stamps in vToDistributeKeys order (:793-825): cell rows, cell columns, raster order inside a cell."""
        g = self.geo
        ks = sorted(self.stamps, key=lambda p: (g.cell(*p), p[1], p[0]))
        return np.array([(x, y, self.stamps[(x, y)]) for x, y in ks], np.int32).reshape(-1, 3)


def _resp(x, y, palette=None):
    v = (x * 7 + y * 13 + (x * y) % 11) % 997
    return 20 + v % 230 if palette is None else palette[v % len(palette)]


def _lattice(geo, keep=lambda x, y: True, palette=None, ox=3, oy=3):
    return {(x, y): _resp(x, y, palette) for y in range(oy, geo.height - 3, 4) for x in range(ox, geo.width - 3, 4)
            if keep(x, y)}


def _frames():
    fr = {}
    fr["empty"] = Frame("empty", G320, {})
    fr["one"] = Frame("one", G320, {(143, 103): 77})
    # the whole 4-px lattice: 71 x 51 = 3,621 stamps, 72 in every full cell (kCandFirst = 7: 65 in overflow slots);
    # few response values, so most nodes hold tied maxima
    lat = _lattice(G320, palette=(40, 90, 140, 200))
    lat[(3, 3)], lat[(7, 3)] = 254, 253                      # response 254 against 253 in one node
    lat[(143, 51)] = 250        # the last key (cell row 1, column 4, last in raster order) of the node [72, 144) x [0, 52)
    quota = {(4, 2): 0, (4, 3): 1, (4, 4): 7, (4, 5): 8}    # cells thinned to 0, 1, kCandFirst and kCandFirst + 1 stamps
    for c, n in quota.items():
        for p in sorted((p for p in lat if G320.cell(*p) == c), key=lambda p: (p[1], p[0]))[n:]:
            del lat[p]
    fr["lattice"] = Frame("lattice", G320, lat)
    # a sparse frame on the 640 roots: keys at the root boundaries (202, 405) and one below, an empty middle root in
    # "roots_gap", a root with one key in "roots_single"
    rb = {(201, 40): 50, (202, 44): 60, (404, 100): 70, (405, 104): 80, (30, 30): 90, (100, 150): 95,
          (300, 60): 100, (310, 160): 105, (500, 50): 110, (560, 170): 115, (204, 10): 120}
    fr["roots"] = Frame("roots", G640, rb)
    fr["roots_gap"] = Frame("roots_gap", G640, {p: r for p, r in rb.items() if not 203 <= p[0] <= 405})
    fr["roots_single"] = Frame("roots_single", G640, {(30, 30): 90, (100, 150): 95, (120, 20): 96, (300, 60): 100,
                                                      (500, 50): 110, (560, 170): 115, (450, 120): 118})
    # DivideNode geometry on the 320 root [0, 288) x [0, 208): xm = 144, ym = 104 for the depth-0 node; the depth-2
    # node [0, 72) x [0, 52) has xm = 36, ym = 26; plus odd widths and heights all the way down
    geo = {(143, 50): 30, (144, 54): 31, (60, 103): 32, (64, 104): 33,
           (35, 10): 34, (36, 14): 35, (10, 25): 36, (14, 26): 37,
           (200, 150): 38, (204, 154): 39, (208, 150): 40, (250, 30): 41, (254, 34): 42, (280, 200): 43,
           (100, 180): 44, (104, 184): 45, (108, 180): 46, (112, 184): 47, (20, 120): 48, (24, 124): 49}
    # two keys of one column, 4 apart in y, inside one depth-5 node (9 x 7 px): no narrower node can hold two stamps
    y0 = next(a for a, b in _edges(0, 208, 5) if b - a == 7 and a > 60)
    geo[(266, y0 + 1)], geo[(266, y0 + 5)] = 50, 51
    fr["geometry"] = Frame("geometry", G320, geo)
    # pseudo-random subsets of the lattice (a fixed arithmetic pattern, no generator state): stop conditions and cuts
    fr["sparse320"] = Frame("sparse320", G320, _lattice(G320, lambda x, y: (x * 31 + y * 17 + x * y) % 13 < 2))
    fr["sparse640"] = Frame("sparse640", G640, _lattice(G640, lambda x, y: (x * 29 + y * 23 + x * y) % 17 < 2))
    fr["half320"] = Frame("half320", G320, _lattice(G320, lambda x, y: (x // 4 + y // 4 * 3 + (x * y) % 5) % 3 != 0,
                                                    palette=(60, 120, 180)))
    fr["big"] = Frame("big", G320, _big())
    return fr


def _split(a, b):
    return a + ((b - a + 1) >> 1)


def _edges(n0, n1, depth):
    """The intervals that `depth` DivideNode halvings (ceil) make of [n0, n1)."""
    e = [(n0, n1)]
    for _ in range(depth):
        e = [p for a, b in e for p in ((a, _split(a, b)), (_split(a, b), b))]
    return e


def _big():
    """More than 2,048 nodes inside the fast-forward (nIni = 1, F = 6): the 32 x 32 depth-5 cells are 9 x 6.5 px; most
    hold a stamp in each of their four depth-6 quadrants, some a fifth in a quadrant wide enough (a two-key depth-6
    node), one cell in sixteen a single stamp (one-key depth-5 nodes, which end the list), six in sixteen none, so
    that round 5 stays in phase 1 (S + 3 E <= N) and round 6 leaves about 2,300 nodes, some hundred with two keys."""
    split = _split
    xs, ys = _edges(0, 288, 5), _edges(0, 208, 5)
    occ = np.zeros((208 + 8, 288 + 8), bool)
    out = {}

    def free(x, y):
        return G320.inside(x, y) and not occ[y + 4 - 3:y + 4 + 4, x + 4 - 3:x + 4 + 4].any()

    def put(x, y):
        occ[y + 4, x + 4] = True
        out[(x, y)] = _resp(x, y, (30, 70, 110, 150, 190, 230))

    for iy, (y0, y1) in enumerate(ys):
        for ix, (x0, x1) in enumerate(xs):
            xm, ym = split(x0, x1), split(y0, y1)
            if iy % 8 in (2, 5, 7):       # empty rows of cells: the rows between them have room for 4 px spacing
                continue
            single = ix % 10 == 9
            for qx0, qx1, qy0, qy1 in ((x0, xm, y0, ym), (xm, x1, y0, ym), (x0, xm, ym, y1), (xm, x1, ym, y1)):
                spots = [(x, y) for y in range(qy0, qy1) for x in range(qx0, qx1) if free(x, y)]
                if not spots:
                    continue
                put(*spots[0])
                if single:
                    break
                if (ix + iy) % 3 == 0:      # a second key in the same depth-6 quadrant where one fits
                    more = [(x, y) for y in range(qy0, qy1) for x in range(qx0, qx1) if free(x, y)]
                    if more:
                        put(*more[0])
    return out


_FRAMES = None


def frames():
    global _FRAMES
    if _FRAMES is None:
        _FRAMES = _frames()
    return _FRAMES


# ---- launch facts restated from the host code (orbgpu_abi.hip geometry, extract_kernels.hip) for the census only
def node_cap(N, nini):
    return (max(N + 8, 4 * nini + 8) + 63) & ~63


def ff_depth(nini, N):
    room, want = 8 * node_cap(N, nini), 6
    for d in range(1, 7):
        if (nini << (2 * d)) >= N:
            want = d
            break
    F = tot = 0
    for d in range(1, want + 1):
        sz = nini << (2 * d)
        if sz > 65536 or tot + sz > room:
            break
        tot += sz
        F = d
    return F


def lds_keys_single(N, geo):
    """octree_lds_keys_whole_cu: the keys that fit one CU's 160 KiB after the node tables (single-frame launch)."""
    room = 160 * 1024 - (node_cap(N, geo.nini) * 64 + 160)
    cand_cap = ((geo.wcell + 1) // 2) * ((geo.hcell + 1) // 2) * geo.ncols * geo.nrows
    return max(0, min((cand_cap + 7) & ~7, (room // 6) & ~7))


def lds_keys_flow(N, geo):
    """build_flow: the dataflow launch's workgroup has 160 KiB less 64 bytes; the keys get what the node tables leave."""
    room = 160 * 1024 - 64 - (node_cap(N, geo.nini) * 64 + 160)
    cand_cap = ((geo.wcell + 1) // 2) * ((geo.hcell + 1) // 2) * geo.ncols * geo.nrows
    return max(0, min((cand_cap + 7) & ~7, (room // 6) & ~7))


def sort_path(N, nini):
    return "binned" if node_cap(N, nini) >= 256 else "pairwise"


class Case:
    def __init__(self, frame, N, items):
        self.frame, self.N, self.items = frames()[frame], N, tuple(items)
        self.name = f"{frame}-N{N}"
        self.geo = self.frame.geo

    def args(self):
        g = self.geo
        return BORDER, BORDER + g.width, BORDER, BORDER + g.height, self.N


KCAND_FIRST = 7
OVERSIZE = 31
CENSUS = (
    "root: keys at int(hX t) - 1 and int(hX t), t = 1, 2", "root: empty middle root", "root: one key (bNoMore)",
    "root: no candidate", "root: one candidate",
    "divide: odd width and odd height", "divide: keys at xm - 1, xm, ym - 1, ym of a depth-1 split",
    "divide: keys at xm - 1, xm, ym - 1, ym of a depth-3 split",
    "divide: two keys of one column still together at depth 5",
    "stop: S == prevSize with S < N", "stop: S == N inside phase 1", "stop: S > N inside phase 1",
    "stop: phase 2 entered with S + 3 nToExpand == N + 1", "stop: S + 3 nToExpand == N stays in phase 1",
    "stop: phase-2 cut lands on N", "stop: phase-2 cut overshoots by 1", "stop: phase-2 cut overshoots by 2",
    "stop: the node that reaches N has 2 children", "stop: the node that reaches N has 3 children",
    "stop: the node that reaches N has 4 children", "stop: a phase-2 round divides everything and goes round again",
    "ff: fin inside the tables", "ff: ph2 inside the tables (quadReady)", "ff: R == F with neither, phase 1 goes on",
    "ff: ph2 at R == F (quadrants counted from the keys)",
) + tuple(f"sort {p}: {t}" for p in ("pairwise", "binned", "oversize")
          for t in ("tie between siblings", "tie between children of different parents", "tie straddles the cut")) + (
    "sort oversize: three or more nodes of >= 31 keys, two of equal size",
) + tuple(f"sort binned: tie straddles {t} ({nw} waves)" for nw in (8, 16)      # 512 threads; the dataflow launch's 1,024
          for t in ("a wave's run", "a 64-node chunk of a run")) + (
    "sort: second phase-2 round with ties (children made by phase 2)",
    "best: tied maximum, cell order first beats raster first", "best: later key strictly larger",
    "best: 254 against 253", "best: node of more than 64 keys, the last key wins",
    "gather: cells with 0, 1, 7, 8 and 72 candidates", "gather: best key in an overflow slot",
    "gather: C > lds_keys (keys in global scratch)", "gather: keys in LDS on the same frame",
    "large: more than 2,048 nodes at the end of the fast-forward, one- and two-key nodes at positions >= 2,048",
    "large: N just below 2,048 on the same frame",
)
# Three items of the issue's census cannot occur and are not here (DESIGN.md section 3.4 has the proofs): a size tie
# between a child of this round and an older undivided node (a phase-2 sort only ever holds nodes created by the round
# before it), a cut that overshoots N by 3 (the list was below N and a division adds at most 3), and a node of
# width 1 with two stamps (a node is never more than about twice as high as wide, and two stamps of one column are
# 4 apart).


def census(case, tr0, out0, out1, cands):
    """The CENSUS items `case` realises; tr0 / out0: trace and result with the pinned tie policy, out1: reversed."""
    got = set()
    g, N = case.geo, case.N
    nini = tr0["nIni"]
    rounds = tr0["rounds"]
    xs = {int(c[0]) for c in cands}
    if nini == 3 and {201, 202, 404, 405} <= xs:
        got.add(CENSUS[0])
    if nini == 3 and tr0["roots"][1][2] == 0 and tr0["roots"][0][2] and tr0["roots"][2][2]:
        got.add(CENSUS[1])
    if any(r[2] == 1 for r in tr0["roots"]) and len(cands) > 1:
        got.add(CENSUS[2])
    if len(cands) == 0:
        got.add(CENSUS[3])
    if len(cands) == 1:
        got.add(CENSUS[4])
    for dv in tr0["divisions"]:
        x0, x1, y0, y1 = dv["rect"]
        if (x1 - x0) % 2 and (y1 - y0) % 2:
            got.add("divide: odd width and odd height")
        kx, ky = {k[0] for k in dv["keys"]}, {k[1] for k in dv["keys"]}
        if {dv["xm"] - 1, dv["xm"]} <= kx and {dv["ym"] - 1, dv["ym"]} <= ky and dv["depth"] in (0, 2):
            got.add(f"divide: keys at xm - 1, xm, ym - 1, ym of a depth-{dv['depth'] + 1} split")
        if dv["depth"] == 5 and len(kx) == 1:     # same x, so 4 apart in y: no deeper node holds both
            got.add("divide: two keys of one column still together at depth 5")
    last = rounds[-1]
    if last["after"] == last["before"] and last["after"] < N and len(cands) > 1:
        got.add("stop: S == prevSize with S < N")
    p1 = [r for r in rounds if r["phase"] == 1]
    p2 = [r for r in rounds if r["phase"] == 2]
    if not p2 and last["after"] == N and last["after"] != last["before"]:
        got.add("stop: S == N inside phase 1")
    if not p2 and last["after"] > N:
        got.add("stop: S > N inside phase 1")
    if p2 and p1[-1]["after"] + 3 * p1[-1]["nToExpand"] == N + 1:
        got.add("stop: phase 2 entered with S + 3 nToExpand == N + 1")
    if any(r["after"] + 3 * r["nToExpand"] == N and r["after"] < N and r["after"] != r["before"] and r["nToExpand"]
           for r in p1[:-1]):
        got.add("stop: S + 3 nToExpand == N stays in phase 1")
    if p2 and p2[-1]["cut"] is not None:
        over = p2[-1]["after"] - N
        got.add("stop: phase-2 cut lands on N" if over == 0 else f"stop: phase-2 cut overshoots by {over}")
        got.add(f"stop: the node that reaches N has {tr0['divisions'][-1]['nonempty']} children")
    if len(p2) > 1:
        got.add("stop: a phase-2 round divides everything and goes round again")
    F, P = ff_depth(nini, N), len(p1)
    if F > 0 and len(cands) > 0:
        fin = not p2
        if fin and P <= F:
            got.add("ff: fin inside the tables")
        if p2 and P < F:
            got.add("ff: ph2 inside the tables (quadReady)")
        if P > F:
            got.add("ff: R == F with neither, phase 1 goes on")
        if p2 and P == F:
            got.add("ff: ph2 at R == F (quadrants counted from the keys)")
    path = sort_path(N, nini)
    differ = out0 != out1
    for ri, r in enumerate(p2):
        srt = r["sorted"]              # (size, seq, depth, parent seq, list position), ascending
        by = {}
        for e in srt:
            by.setdefault(e[0], []).append(e)
        S = r["before"]
        for size, es in by.items():
            if len(es) < 2:
                continue
            paths = ["oversize"] if path == "binned" and size >= OVERSIZE else [path]
            parents = [e[3] for e in es]
            for p in paths:
                if len(set(parents)) < len(parents):
                    got.add(f"sort {p}: tie between siblings")
                if len(set(parents)) > 1:
                    got.add(f"sort {p}: tie between children of different parents")
                j = r["cut"]
                if j is not None and 0 < j and srt[j][0] == size and srt[j - 1][0] == size and differ:
                    got.add(f"sort {p}: tie straddles the cut")
            if ri > 0:
                got.add("sort: second phase-2 round with ties (children made by phase 2)")
            for nw in (8, 16) if path == "binned" and size < OVERSIZE else ():
                pw = -(-S // nw)      # PW: nw = NT / 64 waves, 8 of the 512-thread block, 16 of the dataflow launch's
                runs = {e[4] // pw for e in es}
                if len(runs) > 1:
                    got.add(f"sort binned: tie straddles a wave's run ({nw} waves)")
                for run in runs:
                    if len({(e[4] - run * pw) // 64 for e in es if e[4] // pw == run}) > 1:
                        got.add(f"sort binned: tie straddles a 64-node chunk of a run ({nw} waves)")
        big = [e[0] for e in srt if e[0] >= OVERSIZE]
        if path == "binned" and len(big) >= 3 and len(set(big)) < len(big):
            got.add("sort oversize: three or more nodes of >= 31 keys, two of equal size")
    cell_of = [g.cell(int(c[0]), int(c[1])) for c in cands]
    slot, seen = [], {}
    for c in cell_of:
        slot.append(seen.get(c, 0))
        seen[c] = slot[-1] + 1
    for fn in tr0["final"]:
        bx, by_, br, bi = fn["best"]
        if fn["best_at"] > 0:
            got.add("best: later key strictly larger")
        if fn["count"] > 64 and fn["best_at"] == fn["count"] - 1:
            got.add("best: node of more than 64 keys, the last key wins")
        if slot[bi] >= KCAND_FIRST:
            got.add("gather: best key in an overflow slot")
        if br == 254 and fn.get("has253"):
            got.add("best: 254 against 253")
        if fn.get("raster_other"):
            got.add("best: tied maximum, cell order first beats raster first")
    counts = set(seen.values()) | ({0} if len(seen) < g.ncols * g.nrows else set())
    if {0, 1, 7, 8, 72} <= counts:
        got.add("gather: cells with 0, 1, 7, 8 and 72 candidates")
    C = len(cands)
    room = lambda n: (min(lds_keys_single(n, g), lds_keys_flow(n, g)), max(lds_keys_single(n, g), lds_keys_flow(n, g)))
    same_frame = [n for f, n, _ in _CASES if f == case.frame.name and n != N]
    if C > room(N)[1]:            # in every launch form
        got.add("gather: C > lds_keys (keys in global scratch)")
    elif C <= room(N)[0] and any(C > room(n)[1] for n in same_frame):
        got.add("gather: keys in LDS on the same frame")
    if p1 and F == 6 and P >= 6:
        r6 = p1[5]
        if r6["after"] > 2048 and any(p >= 2048 for p in r6["multi_pos"]) and r6["after"] - 1 not in r6["multi_pos"]:
            got.add(CENSUS[-2])
    # no list position reaches 2,048 here (the list ends at N + 2 at most), on a frame that has the large case too
    if 2048 - 64 <= N < 2048 - 2 and max(r["after"] for r in rounds) < 2048 and \
            any(CENSUS[-2] in solved(Case(case.frame.name, n, ()))[3] for n in same_frame if n > 2048):
        got.add(CENSUS[-1])
    return got


# (frame, N, the census items the case is there for; census() usually finds more in it)
_CASES = (
    ("empty", 50, ("root: no candidate",)),
    ("one", 50, ("root: one candidate", "ff: fin inside the tables")),
    ("roots", 2, ("root: keys at int(hX t) - 1 and int(hX t), t = 1, 2", "stop: S > N inside phase 1")),
    ("roots", 9, ("ff: ph2 at R == F (quadrants counted from the keys)", "sort pairwise: tie straddles the cut")),
    ("roots_gap", 8, ("root: empty middle root", "ff: R == F with neither, phase 1 goes on",
                      "stop: S + 3 nToExpand == N stays in phase 1", "stop: S == prevSize with S < N")),
    ("roots_single", 7, ("root: one key (bNoMore)", "stop: S == N inside phase 1")),
    ("geometry", 11, ("divide: keys at xm - 1, xm, ym - 1, ym of a depth-1 split",
                      "divide: keys at xm - 1, xm, ym - 1, ym of a depth-3 split",
                      "stop: a phase-2 round divides everything and goes round again",
                      "sort: second phase-2 round with ties (children made by phase 2)",
                      "stop: the node that reaches N has 3 children", "stop: phase-2 cut overshoots by 1")),
    ("geometry", 100, ("divide: two keys of one column still together at depth 5", "divide: odd width and odd height")),
    ("sparse320", 64, ("stop: S + 3 nToExpand == N stays in phase 1",)),
    ("sparse640", 10, ("best: tied maximum, cell order first beats raster first",)),
    ("half320", 190, ("sort oversize: tie straddles the cut", "sort oversize: tie between siblings",
                      "sort oversize: tie between children of different parents")),
    ("lattice", 20, ("best: node of more than 64 keys, the last key wins", "best: 254 against 253",
                     "gather: cells with 0, 1, 7, 8 and 72 candidates", "gather: keys in LDS on the same frame",
                     "sort pairwise: tie between siblings", "sort pairwise: tie between children of different parents")),
    ("lattice", 186, ("sort oversize: three or more nodes of >= 31 keys, two of equal size",
                      "sort oversize: tie straddles the cut", "sort binned: tie straddles a wave's run (8 waves)",
                      "sort binned: tie straddles a wave's run (16 waves)")),
    ("lattice", 255, ("stop: phase 2 entered with S + 3 nToExpand == N + 1",
                      "stop: a phase-2 round divides everything and goes round again",
                      "stop: phase-2 cut overshoots by 2", "stop: the node that reaches N has 4 children")),
    ("lattice", 2400, ("gather: C > lds_keys (keys in global scratch)", "ff: ph2 inside the tables (quadReady)",
                       "sort binned: tie straddles a 64-node chunk of a run (8 waves)", "sort binned: tie straddles the cut",
                       "gather: best key in an overflow slot")),
    ("big", 2042, ("large: N just below 2,048 on the same frame", "gather: keys in LDS on the same frame")),
    ("big", 2400, (CENSUS[-2], "gather: C > lds_keys (keys in global scratch)", "stop: phase-2 cut lands on N",
                   "stop: the node that reaches N has 2 children", "sort binned: tie between siblings",
                   "sort binned: tie between children of different parents", "best: later key strictly larger",
                   "sort binned: tie straddles a 64-node chunk of a run (16 waves)")),
)
TIE_ITEMS = tuple(i for i in CENSUS if "tie straddles the cut" in i)   # the two tie policies must give different outputs


def cases():
    return [Case(f, n, items) for f, n, items in _CASES]


_SOLVED = {}


def solved(case):
    """(candidates, (result, trace) pinned, (result, trace) reversed, census items), computed once per case."""
    if case.name not in _SOLVED:
        import octree_ref
        cands = case.frame.candidates()
        keys = [tuple(int(v) for v in k) for k in cands]
        o0, t0 = octree_ref.distribute(keys, *case.args(), False)
        o1, t1 = octree_ref.distribute(keys, *case.args(), True)
        _SOLVED[case.name] = (cands, (o0, t0), (o1, t1), census(case, t0, o0, o1, cands))
    return _SOLVED[case.name]
