"""Named, deterministic descriptor sets that put MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307) at the
edges of k_distinctive's 257-bin histogram (csrc/distinctive.hip: lane l owns bins 5l..5l+4), and the plain reference:
a sort-based median per row, strict first minimum.  Pure numpy; a set is built once and never modified.

Descriptors are planted, not extracted: every descriptor is one random base with a chosen set of bit positions
flipped, so the distance between two of them is the size of the symmetric difference of their sets.

What a set can and cannot do.  Row i's median is the distance of rank k = int(0.5*(N-1)), its own 0 included, so a row
whose median is M has more than N/2 rows at distance >= M.  If the *winning* (smallest) median is M, every row has
that many; two rows that are far from each other then share a third row far from both, and three descriptors have
pairwise distances summing to at most 2*256, so 3M <= 512: no winning median exceeds 170.  Bins 254, 255 and 256 are
therefore planted as the medians of rows that must lose (a complement, and a complement with one and two bits put
back, in front of a majority of one descriptor), and the winning medians are planted at 0, 4, 5, 9, 10 (first and last
bin of lanes 0-2), 64, 65 and at the bound, 170 (lane 34).  By the same bound, reading bin 256 as empty cannot change
the chosen index: the row whose median is 256 loses either way.

Shape of a planted set with winning median B: an outlier row first (farther than B from every other row, so its median
is above B), then three clusters W = base, P = base^S_P, Q = base^S_Q with |S_P| = |S_Q| = B, S_P and S_Q disjoint
(d(P, Q) = 2B), each cluster at most k rows.  A W row then sees its own cluster at 0 and all others at B: median B;
P and Q rows see B or 2B.  The winner is the first row after the outlier whose median is B."""
import collections
import functools

import numpy as np

DSet = collections.namedtuple("DSet", "name desc winner median row_medians items")

ITEMS = (
    *(f"win_bin_{b}" for b in (0, 4, 5, 9, 10, 64, 65, 170)),
    *(f"row_bin_{b}" for b in (254, 255, 256)),
    *(f"n_{n}" for n in (1, 2, 3, 63, 64, 65, 128, 129)),
    "all_identical", "tie_first_and_later_row", "winner_not_first_row", "winner_beyond_lane_stride",
    "nmp_1", "nmp_4", "nmp_5", "empty_between_full",
)


def flipped(base, bits):
    m = np.zeros(256, np.uint8)
    m[list(bits)] = 1
    return base ^ np.packbits(m)


def distance(a, b):
    return int(np.unpackbits(a ^ b).sum())


# ---- the reference
def row_medians(desc):
    """vDists[0.5*(N-1)] of every row after the sort (MapPoint.cc:290-294)."""
    n = len(desc)
    out = []
    for i in range(n):
        row = sorted(distance(desc[i], desc[j]) for j in range(n))
        out.append(row[int(0.5 * (n - 1))])
    return out


def distinctive(desc):
    """(BestIdx, BestMedian, medians) (MapPoint.cc:288-301): strict <, so the first row of the minimum."""
    med = row_medians(desc)
    best_median, best_idx = 2 ** 31 - 1, 0
    for i, m in enumerate(med):
        if m < best_median:
            best_median, best_idx = m, i
    return best_idx, best_median, med


# ---- the sets
def _base(seed):
    return np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)


def _clusters(name, seed, n, b, items, outlier=True):
    """Outlier, then W / P / Q rows interleaved W P Q W P Q ... (so clusters straddle the 64-row lane stride)."""
    base = _base(seed)
    sp = range(0, b)
    sq = range(b, 2 * b) if 2 * b <= 256 else range(256 - b, 256)
    rows = []
    if outlier:
        assert 3 * b + 1 <= 256
        rows.append(flipped(base, range(2 * b, 3 * b + 1)))       # b+1 from W, 2b+1 from P and Q
    kinds = (flipped(base, ()), flipped(base, sp), flipped(base, sq))
    for i in range(n - len(rows)):
        rows.append(kinds[i % 3])
    k = int(0.5 * (n - 1))
    assert (n - len(rows) + 2) // 3 <= k or n < 4, (name, n, k)
    winner = 1 if outlier else 0
    med = [None] * n
    med[winner] = b
    if outlier:      # its own 0, the W rows at b+1, P and Q at 2b+1; rank k is past the W rows
        assert 1 + (n + 1) // 3 <= k
        med[0] = 2 * b + 1
    return DSet(name, np.stack(rows), winner, b, med, items)


def _build():
    s = []
    a = _base(1)
    # N = 1, 2, 3
    s.append(DSet("n1", a[None].copy(), 0, 0, [0], ("n_1",)))
    s.append(DSet("n2", np.stack([a, flipped(a, range(7))]), 0, 0, [0, 0], ("n_2",)))   # k = 0: every median is 0
    # rows b, a, c with d(a,b) = 9, d(a,c) = 5, d(b,c) = 14; k = 1: medians 9, 5, 5; rows 1 and 2 tie, row 1 wins
    s.append(DSet("n3", np.stack([flipped(a, range(9)), a, flipped(a, range(9, 14))]), 1, 5, [9, 5, 5],
                  ("n_3", "tie_first_and_later_row")))
    s.append(_clusters("n63_bin4", 2, 63, 4, ("n_63", "win_bin_4", "winner_not_first_row")))
    s.append(_clusters("n64_bin5", 3, 64, 5, ("n_64", "win_bin_5")))
    s.append(_clusters("n65_bin9", 4, 65, 9, ("n_65", "win_bin_9")))
    s.append(_clusters("n128_bin10", 5, 128, 10, ("n_128", "win_bin_10")))
    s.append(_clusters("n129_bin64", 6, 129, 64, ("n_129", "win_bin_64")))
    s.append(_clusters("n64_bin65", 7, 64, 65, ("win_bin_65",), outlier=False))
    s.append(_clusters("n65_bin170", 8, 65, 170, ("win_bin_170",), outlier=False))
    # all identical: every distance 0
    s.append(DSet("identical129", np.repeat(_base(9)[None], 129, 0), 0, 0, [0] * 129, ("all_identical", "win_bin_0")))
    # complement, complement with one and two bits put back, then 60 copies of a: the three lose with medians
    # 256, 255, 254 (k = 31: three distances <= 2, then 60 times the distance to a); a rows: median 0, row 3 wins
    b = _base(10)
    rows = [flipped(b, range(256)), flipped(b, range(1, 256)), flipped(b, range(2, 256))] + [b] * 60
    s.append(DSet("complements63", np.stack(rows), 3, 0, [256, 255, 254] + [0] * 60,
                  ("row_bin_256", "row_bin_255", "row_bin_254")))
    # the winner alone beyond the 64-row stride: 100 rows of three far clusters (medians >= 40), then at row 100 the
    # one row that is within 20 of all of them (W P Q at pairwise 40, the centre c at 20 from each)
    c = _base(11)
    kinds = [flipped(c, range(0, 20)), flipped(c, range(20, 40)), flipped(c, range(40, 60))]
    rows = [kinds[i % 3] for i in range(100)] + [c] + [kinds[i % 3] for i in range(28)]
    s.append(DSet("late_winner129", np.stack(rows), 100, 20, [40] * 100 + [20] + [40] * 28,
                  ("winner_beyond_lane_stride",)))
    return s


@functools.lru_cache(maxsize=None)
def sets():
    out = {d.name: d for d in _build()}
    for d in out.values():
        d.desc.setflags(write=False)
    return out


EMPTY = np.zeros((0, 32), np.uint8)

# one call's map points: names of sets, None = a map point without observations.  One block holds four map points
# (one per wave): nmp = 1 leaves three waves idle, 4 fills the block, 5 starts a second block with one wave.
BATCHES = {
    "nmp_1": ("n65_bin9",),
    "nmp_4": ("n63_bin4", "n1", "complements63", "n129_bin64"),
    "nmp_5": ("n64_bin5", "n3", "n128_bin10", "n2", "late_winner129"),
    "empty_between_full": ("identical129", None, "n65_bin170", None, None, "n64_bin65", None),
}
