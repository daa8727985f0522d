"""Named, deterministic inputs that put every decision of ORBmatcher::SearchForTriangulation (ORBmatcher.cc:657-823)
at its edge.  Pure numpy; tests/test_triangulation_cases.py checks on the CPU that tests/triangulation_ref.py and the
oracle agree and that every planted decision is realised in the reference trace; tests/test_gpu_triangulation_cases.py
runs the same arrays through k_triangulation, single and batched.

How the numbers were chosen.  F12 = [[1, 0, 0], [0, 1, 0], [-97, -96, -700]] gives the epipolar line of a KF1 keypoint
(x1, y1) as a = x1 - 97, b = y1 - 96, c = -700.  Every ordinary query sits at (100, 100): a = 3, b = 4, den = 25, and
the line passes through P = (140, 70), so a candidate at P + (dx, dy) has num = 3 dx + 4 dy and dsqr = num^2 / 25.
Level 0 has sigma2 = 1 (3.84 * sigma2 = 3.84): num = 9 gives 3.24 (inside), num = 10 gives 4.0 (outside).  Level 1 has
sigma2 = 1.5625 (the limit is 5.9999...): num = 12 gives 5.76 (inside), num = 13 gives 6.76 (outside).  The query at
(97, 96) has a = b = 0: den == 0.  The epipole is (94, 92): a candidate at (100, 100) is at squared distance
36 + 64 = 100 = 100 * scaleFactor[0], at (104, 97) on level 1 at 100 + 25 = 125 = 100 * 1.25; one pixel nearer they
are inside.  P is far from the epipole, so the ordinary candidates pass that gate.

Margin against the fused form (tools/ref_flags_probe.cpp, csrc/hamming_kernels.hip: den = fma(a, a, b*b),
num = fma(b, y2, a*x2) + c): every coordinate, every entry of F12 and every product and sum above is an integer below
2^20, exact in float, so the fused and unfused forms compute identical a, b, c, num and den, and dsqr is one
division of the same operands.  The nearest planted dsqr is 0.16 away from its limit.

Descriptors are planted (a partner at distance d has exactly d bits flipped); fillers are random.  Edge nodes use
angle 0; the rotation case has one pair per node.  A case is built once and never modified."""
import collections
import functools

import numpy as np

import triangulation_ref as ref
from planted_tools import ROT_TIED, ROT_TIED_EXPECTED, Builder

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
F12 = np.array([[1, 0, 0], [0, 1, 0], [-97, -96, -700]], np.float32)
EX, EY = 94.0, 92.0
SCALE2 = np.array([1.0, 1.25, 1.5625], np.float32)
SIGMA2 = np.array([1.0, 1.5625, 2.44140625], np.float32)
Q, P = (100.0, 100.0), (140.0, 70.0)

Case = collections.namedtuple("Case", "name desc1 kps1 mp1 ur1 fv1 desc2 kps2 mp2 ur2 fv2 plants rot fillers")
# best / best_stereo: the expected bestIdx2 (-1: none) with bOnlyStereo false / true; None = not pinned
Plant = collections.namedtuple("Plant", "item idx1 best best_stereo")

ITEMS = (
    "tie_last_wins_across_lanes", "tie_beyond_64", "tie_within_one_stride_pass", "dist_50", "dist_51", "epipole_equal_level0", "epipole_inside_level0",
    "epipole_equal_level1", "epipole_inside_level1", "epipole_gate_skipped_stereo1", "epipole_gate_skipped_stereo2",
    "dsqr_below_level0", "dsqr_above_level0", "dsqr_below_level1", "dsqr_above_level1", "den_zero",
    "closer_candidate_fails_line", "closer_candidate_fails_epipole", "only_stereo_query_mono", "only_stereo_train_mono",
    "train_has_map_point", "query_has_map_point", "train_matched_twice", "candidates_above_64",
    "rot_negative_wrap", "rot_bin_30_to_0", "rot_round_half", "maxima_first_second_tied", "maxima_third_tied_first_wins",
    "maxima_third_at_cutoff_kept", "culled_pair_removed",
)


class _T(Builder):
    def __init__(self, name, seed):
        super().__init__(name, seed, 0.0)
        self.kp = ([], [])
        self.ur = ([], [])

    def feat(self, side, node, desc, xy, octave=0, mp=0, ur=-1.0, angle=0.0, pos=None):
        i = self.add(side, node, desc, mp=mp, angle=angle, pos=pos)
        self.kp[side - 1].append((xy[0], xy[1], 31.0, angle, 50.0, octave, -1))
        self.ur[side - 1].append(ur)
        return i

    def q(self, node, xy=Q, **kw):
        d = self.rand()
        return self.feat(1, node, d, xy, **kw), d

    def c(self, node, d, dist, off=(0, 0), base=P, at=0, **kw):
        """A candidate at base + off whose descriptor differs from d in bits [at, at + dist)."""
        return self.feat(2, node, self.flip(d, range(at, at + dist)), (base[0] + off[0], base[1] + off[1]), **kw)

    def plant(self, item, idx1, best=None, best_stereo=None):
        self.plants.append(Plant(item, idx1, best, best_stereo))

    def done(self, rot=None):
        a = lambda x, t: np.ascontiguousarray(np.array(x, t))
        c = Case(self.name, a(self.d[0], np.uint8).reshape(-1, 32), a(self.kp[0], KP_DTYPE), a(self.mp[0], np.uint8),
                 a(self.ur[0], np.float32), {k: list(v) for k, v in self.fv[0].items()},
                 a(self.d[1], np.uint8).reshape(-1, 32), a(self.kp[1], KP_DTYPE), a(self.mp[1], np.uint8),
                 a(self.ur[1], np.float32), {k: list(v) for k, v in self.fv[1].items()}, tuple(self.plants), rot, tuple(self.fillers))
        for x in (c.desc1, c.kps1, c.mp1, c.ur1, c.desc2, c.kps2, c.mp2, c.ur2):
            x.setflags(write=False)
        return c


def _edges():
    b = _T("edges", 31)
    # 70 candidates; positions 3 and 68 tie at 20 bits and both pass every gate: the later one stays (:738 skips
    # only dist > bestDist).  Fillers are random descriptors, far above TH_LOW
    i, d = b.q(1)
    for _ in range(68):
        b.fillers.append(b.feat(2, 1, b.rand(), P))
    b.c(1, d, 20, at=0, pos=3)
    late = b.c(1, d, 20, at=20, off=(4, -3), pos=68)
    assert len(b.fv[1][1]) == 70 and b.fv[1][1][68] == late
    b.plant("tie_last_wins_across_lanes", i, late, -1)
    b.plant("tie_beyond_64", i, late, -1)
    b.plant("candidates_above_64", i, late, -1)
    # the same tie at positions 3 and 40 of 50 candidates: one pass of the 64-lane stride, different lanes, so only
    # the reduction across lanes orders them
    i, d = b.q(22)
    for _ in range(48):
        b.fillers.append(b.feat(2, 22, b.rand(), P))
    b.c(22, d, 20, at=0, pos=3)
    late = b.c(22, d, 20, at=20, off=(4, -3), pos=40)
    assert len(b.fv[1][22]) == 50 and b.fv[1][22][40] == late
    b.plant("tie_within_one_stride_pass", i, late, -1)
    i, d = b.q(2)
    b.plant("dist_50", i, b.c(2, d, 50), -1)
    i, d = b.q(3)
    b.c(3, d, 51)
    b.plant("dist_51", i, -1, -1)
    # the epipole gate (:743-748): the query is at the candidate's own position, so the line test passes (num = 0 for
    # (100, 100); 3*4 + 4*(-3) = 0 for (104, 97))
    i, d = b.q(4)
    b.plant("epipole_equal_level0", i, b.c(4, d, 5, base=(100.0, 100.0)), -1)
    i, d = b.q(5)
    b.c(5, d, 5, base=(100.0, 99.0))
    b.plant("epipole_inside_level0", i, -1, -1)
    i, d = b.q(6)
    b.plant("epipole_equal_level1", i, b.c(6, d, 5, base=(104.0, 97.0), octave=1), -1)
    i, d = b.q(7)
    b.c(7, d, 5, base=(104.0, 96.0), octave=1)
    b.plant("epipole_inside_level1", i, -1, -1)
    # stereo on one side only: the gate is not applied, the candidate inside the radius is taken
    i, d = b.q(8, ur=80.0)
    b.plant("epipole_gate_skipped_stereo1", i, b.c(8, d, 5, base=(100.0, 99.0)), -1)
    i, d = b.q(9)
    b.plant("epipole_gate_skipped_stereo2", i, b.c(9, d, 5, base=(100.0, 99.0), ur=80.0), -1)
    # 3.84 * sigma2 on either side, levels 0 and 1: (3, 0) -> num 9; (2, 1) -> 10; (4, 0) -> 12; (3, 1) -> 13
    for node, item, off, octave, hit in ((10, "dsqr_below_level0", (3, 0), 0, True), (11, "dsqr_above_level0", (2, 1), 0, False),
                                         (12, "dsqr_below_level1", (4, 0), 1, True), (13, "dsqr_above_level1", (3, 1), 1, False)):
        i, d = b.q(node)
        t = b.c(node, d, 5, off=off, octave=octave)
        b.plant(item, i, t if hit else -1, -1)
    i, d = b.q(14, xy=(97.0, 96.0))
    b.c(14, d, 5)
    b.plant("den_zero", i, -1, -1)
    # a closer candidate that fails a gate must not lower bestDist: [30 passes, 10 fails, 25 passes] -> the 25
    i, d = b.q(15)
    b.c(15, d, 30, at=0)
    b.c(15, d, 10, at=30, off=(2, 1))
    b.plant("closer_candidate_fails_line", i, b.c(15, d, 25, at=40, off=(4, -3)), -1)
    i, d = b.q(16)
    b.c(16, d, 30, at=0)
    b.c(16, d, 10, at=30, base=(100.0, 99.0))
    b.plant("closer_candidate_fails_epipole", i, b.c(16, d, 25, at=40, off=(4, -3)), -1)
    # bOnlyStereo: a mono query is not visited; a mono train is skipped in favour of a farther stereo one
    i, d = b.q(17, ur=50.0)
    near = b.c(17, d, 5)
    far = b.c(17, d, 40, at=5, ur=60.0)
    b.plant("only_stereo_train_mono", i, near, far)
    i, d = b.q(18)
    b.plant("only_stereo_query_mono", i, b.c(18, d, 5, ur=60.0), -1)
    i, d = b.q(19)
    b.c(19, d, 0, mp=1)
    b.plant("train_has_map_point", i, b.c(19, d, 12), -1)
    i, d = b.q(20, mp=1)
    b.c(20, d, 0)
    b.plant("query_has_map_point", i, -1, -1)
    # vbMatched2 is never set (:677): two queries of one node both get the same train
    i, d = b.q(21, ur=50.0)
    t = b.c(21, d, 4, ur=60.0)
    j = b.feat(1, 21, b.flip(d, range(100, 106)), Q, ur=50.0)
    b.plant("train_matched_twice", i, t, t)
    b.plant("train_matched_twice", j, t, t)
    return b.done()


def _rot():
    pairs = ROT_TIED
    b = _T("rot_tied", 32)
    for n, (a1, a2) in enumerate(pairs):
        i, d = b.q(n, angle=a1)
        t = b.c(n, d, 5, angle=a2)
        if n == len(pairs) - 1:
            b.plant("culled_pair_removed", i, t, -1)       # the loop's answer; the histogram then removes the pair
    return b.done(ROT_TIED_EXPECTED)


@functools.lru_cache(maxsize=None)
def cases():
    return {c.name: c for c in (_edges(), _rot())}


CASES = ("edges", "rot_tied")


def reversed_lists(c):
    return c._replace(fv2={k: v[::-1] for k, v in c.fv2.items()})


def expected(c, only_stereo):
    return ref.search_for_triangulation(True, only_stereo, c.desc1, c.kps1, c.mp1, c.ur1, c.fv1, c.desc2, c.kps2, c.mp2,
                                        c.ur2, c.fv2, F12, EX, EY, SCALE2, SIGMA2)
