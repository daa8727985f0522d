"""Named, deterministic inputs that put every decision of the window matchers (SearchForInitialization,
ORBmatcher.cc:405-520, and BirdviewMatch(const Frame&, const Frame&), :1788-1899) at its edge.  Pure numpy;
tests/test_window_cases.py checks on the CPU that tests/window_ref.py and the oracle agree and that every planted
decision is realised in the reference trace; tests/test_gpu_window_cases.py runs the same arrays through the list form
(k_topk) and the grid form (k_window_topk) and the host replay.

One case.  The frame is 512 x 384 with bounds (0, 512, 0, 384), so a grid cell is 8 x 8 pixels and 1/8 is exact; the
window radius is 16; all coordinates are integers, so every float expression of the grid lookup is exact.  Each
decision lives in a region of its own: region k has its centre at (32 + 64 (k % 8), 32 + 64 (k // 8)), 64 pixels from
the next, so no window sees another region.  Queries (F1) and candidates (F2) are given as offsets from the centre.
Descriptors are planted (a partner at distance d has exactly d bits flipped); fillers are random (the CPU test asserts
more than 80 bits from every query of their region).  All angles are 0: the rotation histogram (shared code with the
BoW replays, pinned in tests/bow_cases.py) culls nothing.  F1's order is the visit order.

A case is built once and never modified."""
import collections
import functools

import numpy as np

import window_ref as ref
from planted_tools import Builder

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
BOUNDS = (0.0, 512.0, 0.0, 384.0)
R = 16.0
NNRATIO = 0.5

Case = collections.namedtuple("Case", "desc1 kps1 desc2 kps2 plants fillers region1 region2")
# init / window: (outcome, bestDist, bestDist2, bestIdx2) with level0_only on / off; final: vnMatches12[i1] (both)
Plant = collections.namedtuple("Plant", "item i1 init window final")

ITEMS = (
    "th_low_50", "th_low_51", "ratio_equal", "ratio_below", "one_candidate", "second_best_ties_best",
    "second_best_ties_best_beyond_64", "earlier_match_replaced", "later_better_match_replaces", "blocked_at_equal_distance",
    "level0_only_query_skipped", "candidate_on_another_level", "empty_window", "window_off_the_grid",
    "rect_edge_equal_excluded", "rect_edge_one_inside", "candidates_above_64", "best_beyond_lane_stride",
    "topk_list_exhausted_by_matched_distance",
)


def centre(k):
    return 32.0 + 64.0 * (k % 8), 32.0 + 64.0 * (k // 8)


class _W:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.d, self.kp, self.region = ([], []), ([], []), ([], [])
        self.plants, self.fillers = [], []

    def rand(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    flip = staticmethod(Builder.flip)

    def feat(self, side, k, desc, off=(0, 0), octave=0, xy=None):
        cx, cy = centre(k)
        x, y = (cx + off[0], cy + off[1]) if xy is None else xy
        self.d[side - 1].append(desc)
        self.kp[side - 1].append((x, y, 31.0, 0.0, 50.0, octave, -1))
        self.region[side - 1].append(k)
        return len(self.d[side - 1]) - 1

    def q(self, k, desc=None, **kw):
        desc = self.rand() if desc is None else desc
        return self.feat(1, k, desc, **kw), desc

    def c(self, k, d, dist, off, at=0, **kw):
        return self.feat(2, k, self.flip(d, range(at, at + dist)), off, **kw)

    def plant(self, item, i1, init=None, window="same", final=None):
        self.plants.append(Plant(item, i1, init, init if window == "same" else window, final))

    def done(self):
        a = lambda x, t: np.ascontiguousarray(np.array(x, t))
        c = Case(a(self.d[0], np.uint8).reshape(-1, 32), a(self.kp[0], KP_DTYPE), a(self.d[1], np.uint8).reshape(-1, 32),
                 a(self.kp[1], KP_DTYPE), tuple(self.plants), tuple(self.fillers), tuple(self.region[0]),
                 tuple(self.region[1]))
        for x in (c.desc1, c.kps1, c.desc2, c.kps2):
            x.setflags(write=False)
        return c


A, D, RT, LV, EM = ref.ACCEPTED, ref.DIST, ref.RATIO, ref.LEVEL, ref.EMPTY
IMAX = ref.INT_MAX


@functools.lru_cache(maxsize=None)
def case():
    b = _W(41)
    i, d = b.q(0)
    t = b.c(0, d, 50, (1, 0))
    b.c(0, d, 200, (2, 0), at=50)
    b.plant("th_low_50", i, (A, 50, 200, t), final=t)
    i, d = b.q(1)
    t = b.c(1, d, 51, (1, 0))
    b.c(1, d, 200, (2, 0), at=51)
    b.plant("th_low_51", i, (D, 51, 200, t), final=-1)
    i, d = b.q(2)
    t = b.c(2, d, 20, (1, 0))
    b.c(2, d, 40, (2, 0), at=20)
    b.plant("ratio_equal", i, (RT, 20, 40, t), final=-1)                 # 20 < 40.0f * 0.5f is false
    i, d = b.q(3)
    t = b.c(3, d, 19, (1, 0))
    b.c(3, d, 40, (2, 0), at=19)
    b.plant("ratio_below", i, (A, 19, 40, t), final=t)
    i, d = b.q(4)
    t = b.c(4, d, 40, (-3, 5))
    b.plant("one_candidate", i, (A, 40, IMAX, t), final=t)              # bestDist2 stays INT_MAX
    i, d = b.q(5)
    t = b.c(5, d, 10, (-9, 0))
    b.c(5, d, 10, (9, 0), at=10)
    b.plant("second_best_ties_best", i, (RT, 10, 10, t), final=-1)
    # region 6: t is taken by qa at 20, then by qb at 10 (vMatchedDistance[t] = 20 > 10: still a candidate), which
    # unsets qa through vnMatches21; qc is at 10 too (10 <= 10: blocked) and takes u
    base = b.rand()
    t = b.feat(2, 6, base, (0, 0))
    ia, _ = b.q(6, b.flip(base, range(0, 20)), off=(1, 0))
    ib, _ = b.q(6, b.flip(base, range(30, 40)), off=(0, 1))
    qc = b.flip(base, range(50, 60))
    ic, _ = b.q(6, qc, off=(1, 1))
    u = b.feat(2, 6, b.flip(qc, range(100, 130)), (2, 2))
    b.plant("earlier_match_replaced", ia, (A, 20, 60, t), final=-1)    # u is 20 + 10 + 30 bits from qa, 10 + 40 from qb
    b.plant("later_better_match_replaces", ib, (A, 10, 50, t), final=t)
    b.plant("blocked_at_equal_distance", ic, (A, 30, IMAX, u), final=u)
    # level0_only: a level-1 query is skipped by SearchForInitialization and matched by the window form
    i, d = b.q(7, octave=1)
    t = b.c(7, d, 5, (1, 0), octave=1)
    b.plant("level0_only_query_skipped", i, (LV, None, None, -1), (A, 5, IMAX, t), final=None)
    i, d = b.q(8)
    b.c(8, d, 0, (1, 0), octave=1)
    t = b.c(8, d, 30, (2, 0))
    b.plant("candidate_on_another_level", i, (A, 30, IMAX, t), final=t)
    i, d = b.q(9)
    b.plant("empty_window", i, (EM, None, None, -1), final=-1)
    i, d = b.q(10, xy=(700.0, 100.0))                                     # (700 - 16) / 8 = 85.5: past column 63
    b.plant("window_off_the_grid", i, (EM, None, None, -1), final=-1)
    # the rectangle's fabs(..) < r: exact copies at distance r in x or y are outside, the partner at r - 1 is inside
    i, d = b.q(11)
    for off in ((16, 0), (0, 16), (-16, 0), (0, -16), (16, 16)):
        b.c(11, d, 0, off)
    t = b.c(11, d, 12, (15, -15))
    b.plant("rect_edge_equal_excluded", i, (A, 12, IMAX, t), final=t)
    b.plant("rect_edge_one_inside", i, (A, 12, IMAX, t), final=t)
    # region 12: 90 candidates in one window.  Q's eight nearest (10..17 bits) are each matched at 3 bits by an
    # earlier query, so all eight are blocked when Q's turn comes and its top-8 list holds nothing admissible while
    # 82 others remain: ranked again, Q takes t8 (30) with t9 (62) second
    Q = b.rand()
    spots = [(x, y) for x in range(-15, 16, 3) for y in range(-15, 16, 3)]      # 121 distinct offsets
    order = b.rng.permutation(len(spots))
    sizes, at, near = [10 + k for k in range(8)] + [30, 62], 0, []
    for s in sizes:
        near.append(b.flip(Q, range(at, at + s)))
        at += s
    for n in range(80):
        b.fillers.append(b.feat(2, 12, b.rand(), spots[order[n]]))
    tn = [b.feat(2, 12, near[k], spots[order[80 + k]] if k != 7 else (15, 15)) for k in range(10)]
    assert spots[-1] == (15, 15)                   # t7 sits in the window's last cell: late in vIndices2
    for k in range(8):
        i, _ = b.q(12, b.flip(near[k], range(200 + 3 * k, 203 + 3 * k)))
        if k == 7:
            b.plant("best_beyond_lane_stride", i, (A, 3, 50, tn[7]), final=tn[7])
    i, _ = b.q(12, Q)
    b.plant("topk_list_exhausted_by_matched_distance", i, (A, 30, 62, tn[8]), final=tn[8])
    b.plant("candidates_above_64", i, (A, 30, 62, tn[8]), final=tn[8])
    # region 13: the tied pair in the window's first and last cell, 70 fillers between them
    i, d = b.q(13)
    t = b.c(13, d, 10, (-15, -15))
    for n in range(70):
        off = spots[order[n]]
        b.fillers.append(b.feat(2, 13, b.rand(), off if off not in ((-15, -15), (15, 15)) else (0, 1)))
    b.c(13, d, 10, (15, 15), at=10)
    b.plant("second_best_ties_best_beyond_64", i, (RT, 10, 10, t), final=-1)
    return b.done()


def grid():
    c = case()
    return ref.Grid(c.kps2, *BOUNDS)


@functools.lru_cache(maxsize=None)
def candidates(reverse=False):
    lists = ref.candidate_lists(grid(), case().kps1, R)
    return tuple(tuple(l[::-1]) if reverse else tuple(l) for l in lists)


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([i for l in lists for i in l], np.int32)


@functools.lru_cache(maxsize=None)
def expected(level0_only, reverse=False):
    c = case()
    return ref.window_match(NNRATIO, True, level0_only, c.desc1, c.kps1, c.desc2, c.kps2, candidates(reverse))
