"""Descriptor slots with planted structure for the all-pairs Hamming top-2 (k_top2_mfma / k_top2b_merge,
csrc/hamming_top2.hip), and the exact reference.  Pure numpy: the builder and the reference run anywhere
(tests/test_top2_cases.py); tests/test_gpu_top2_stages.py uploads the slots and compares exactly.

A case is a set of frame pairs (query frame 2k, train frame 2k + 1) in the layout of an extraction batch:
desc[frame, row, 32] with counts[frame] live rows of kp_cap.  Background descriptors are uniform random (pairwise
distances near 128).  A plant takes one query row i and train rows a < b (and c) that no other plant of the frame
uses and sets t[a] = q[i] ^ flips(d_a), ... with every planted distance <= 40, so the expected (best, index, second)
of query i is known by construction; tests/test_top2_cases.py asserts that the reference returns exactly that for
every plant.  Rows past counts[frame] hold copies of the partner frame's live rows (distance 0 if ever read)."""
import collections
import functools

import numpy as np

TILE = 32    # trains per MFMA tile
STAGE = 64   # trains per stage (one LDS buffer)
SENTINEL = (257, -1, 257)
PREFILL = 0x5A5A5A5A

# Launch shapes.  slices = what orb_hamming_top2_slices(npairs, kp_cap, kp_cap) must return, slice_len = the only
# multiple of 64 that covers kp_cap in that many slices, min_stages = stages the longest slice must have (the
# steady-state loop of k_top2_mfma runs stages - 1 times; three stages reuse an LDS buffer).
Shape = collections.namedtuple("Shape", "name kp_cap npairs slices slice_len min_stages")
SHAPES = (
    # one slice of 6 stages, written directly; last stage 10 live rows (tile 1 masked whole); second query block 74
    Shape("direct_330x1024", 330, 1024, 1, 384, 3),
    # slices of 256, 256, 128 merged by k_top2b_merge; 3 x 3 x 300 = 2700 blocks (not a multiple of 8)
    Shape("merge_640x300", 640, 300, 3, 256, 3),
    # four slices of 128 (two stages each, the last one stage); the partial buffer is sized for six
    Shape("merge_448x171", 448, 171, 4, 128, 2),
)
SHAPE_BY_NAME = {s.name: s for s in SHAPES}

VARIANTS = ("tie", "later_better", "earlier_better", "third_row", "triple_tie", "copies")
# every (a, b) position kind, tightest (fewest candidate rows) first; the last two exist only for sliced shapes
POSITIONS = ("b_last", "slice_boundary", "first_last_stage", "tile0_tile1", "adjacent_stages", "stage_j_j2",
             "first_last_slice", "same_tile_other_half", "same_tile_same_half")
SLICED_ONLY = ("slice_boundary", "first_last_slice")

Plant = collections.namedtuple("Plant", "qframe tframe qi cls pos a b c expect")
Case = collections.namedtuple("Case", "shape desc counts qf tf combos combo_of_pair plants")


def top2_numpy(dq, dt):
    """(best, first argmin, second) of the 256-bit Hamming distances, DescriptorDistance
    (ORBmatcher.cc:1647-1663) as a popcount of the XOR of four u64 words.  second counts multiplicity (two trains
    at the best distance: second == best); no train: 257 / -1 / 257, one train: second 257."""
    a = np.ascontiguousarray(dq).view(np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(dt).view(np.uint64).reshape(-1, 4)
    if len(b) == 0:
        return (np.full(len(a), SENTINEL[0], np.int32), np.full(len(a), SENTINEL[1], np.int64),
                np.full(len(a), SENTINEL[2], np.int32))
    D = np.zeros((len(a), len(b)), np.int32)
    for w in range(4):
        D += np.bitwise_count(a[:, w, None] ^ b[None, :, w]).astype(np.int32)
    srt = np.partition(D, 1, axis=1) if D.shape[1] > 1 else D
    return D.min(1), D.argmin(1), srt[:, 1] if D.shape[1] > 1 else np.full(len(a), 257)


def frame_counts(kp_cap):
    return [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, kp_cap - 1, kp_cap]


def flips(rng, d):
    """A 32-byte mask with exactly d distinct bits set."""
    bits = np.zeros(256, np.uint8)
    bits[rng.choice(256, d, replace=False)] = 1
    return np.packbits(bits)


def position_candidates(pos, nt, L):
    """Every (a, b), a < b < nt, of one position kind for a train set of nt rows cut into slices of L rows."""
    out = []
    last = nt - 1
    if pos == "b_last":
        # a in another stage than the last row where there is one
        out = [(a, last) for a in (7, 40, 70, 100, 135, 170, 200, 230, 3, 1, 0) if a < last]
    elif pos == "slice_boundary":
        out = [(k - 1, k) for k in range(L, nt, L)]
    elif pos == "first_last_stage":
        # a in the launch's first stage, b a live row of the last stage, which must be cut short by nt
        ls = last // STAGE
        if nt % STAGE and ls > 0:
            out = [(a, b) for b in range(ls * STAGE, nt) for a in (5 + b % 23, 37 + b % 19)]
    elif pos == "tile0_tile1":
        out = [(s + 31, s + 32) for s in range(0, nt, STAGE) if s + 32 < nt]
    elif pos == "adjacent_stages":
        # rows 63 | 64 of one slice: the other LDS buffer
        out = [(s - 1, s) for s in range(STAGE, nt, STAGE) if s % L]
    elif pos == "stage_j_j2":
        # the same LDS buffer, reused; inside one slice wherever a slice has three stages
        for s in range(0, nt, STAGE):
            for x in (6, 21, 45, 58):
                a, b = s + x, s + 2 * STAGE + x
                if b < nt and (L < 3 * STAGE or a // L == b // L):
                    out.append((a, b))
    elif pos == "first_last_slice":
        if last // L > 0:
            lo = last // L * L
            out = [(a, b) for b in range(lo + 2, nt, 7) for a in (11 + b % 17, 44 + b % 13, 66 + b % 29) if a < L]
    elif pos == "same_tile_other_half":
        # rows r and r ^ 4: the two lane halves, combined by the closing __shfl_xor(..., 32)
        out = [(tb + r, tb + r + 4) for tb in range(0, nt, TILE) for r in (3, 10, 17, 24) if tb + r + 4 < nt]
    elif pos == "same_tile_same_half":
        out = [(tb + r1, tb + r2) for tb in range(0, nt, TILE) for r1, r2 in ((1, 9), (2, 19), (5, 14), (20, 29))
               if tb + r2 < nt]
    else:
        raise KeyError(pos)
    return out


def _plant_frame_pair(rng, k, q, t, nq, nt, L, sliced, skip):
    """Plants of frame pair k: one per (variant, position) where rows are left.  Writes the train rows into t
    and returns the Plant list.  Query row skip is left alone."""
    plants = []
    free_t = np.ones(nt, bool)
    qrows = [i for i in rng.permutation(nq) if i != skip]
    want = []
    for pos in POSITIONS:
        if pos in SLICED_ONLY and not sliced:
            continue
        cand = position_candidates(pos, nt, L)
        for v in range(len(VARIANTS)):
            cls = VARIANTS[(v + k) % len(VARIANTS)]   # rotated: each variant gets the scarce rows in some frame pair
            if not qrows:
                break
            n = len(cand)
            for j in range(n):
                a, b = cand[(j + (v + k) * 5) % n]    # (different variants start in different stages)
                if free_t[a] and free_t[b]:
                    free_t[a] = free_t[b] = False
                    want.append((qrows.pop(), cls, pos, a, b))
                    break
    for qi, cls, pos, a, b in want:
        c = -1
        if cls in ("third_row", "triple_tie"):
            left = np.flatnonzero(free_t)
            if len(left) == 0:
                free_t[a] = free_t[b] = True   # (rows go back to the background)
                continue
            c = int(rng.choice(left))
            free_t[c] = False
        d = int(rng.integers(0, 37))
        if cls == "tie":
            dist, expect = (d, d), (d, a, d)
        elif cls == "later_better":
            dist, expect = (d + 1, d), (d, b, d + 1)
        elif cls == "earlier_better":
            dist, expect = (d, d + 1), (d, a, d + 1)
        elif cls == "third_row":
            w = d + int(rng.integers(1, 4))
            dist, expect = (d, w, w), (d, a, w)
        elif cls == "triple_tie":
            dist, expect = (d, d, d), (d, min(a, b, c), d)
        else:   # copies: two exact copies of the query
            dist, expect = (0, 0), (0, a, 0)
        for row, dd in zip((a, b, c), dist):
            t[row] = q[qi] ^ flips(rng, dd)
        plants.append(Plant(2 * k, 2 * k + 1, int(qi), cls, pos, a, b, c, expect))
    return plants


def _frame_pair_sizes(cap):
    """(nq, nt) per frame pair: six full-size pairs (every variant gets the scarce positions once), every count
    as a train count against the counts in reverse as query counts, and full query frames against the train
    counts that cut a stage short or end on a stage."""
    s = frame_counts(cap)
    sizes = [(cap, cap), (cap, cap - 1), (cap - 1, cap), (cap, cap - 1), (cap, cap), (cap, cap - 1)]
    sizes += [(s[len(s) - 1 - i], nt) for i, nt in enumerate(s)]
    sizes += [(cap, 65), (cap, 129), (cap, 193), (cap, 257), (cap - 1, 127), (cap - 1, 192)]
    return sizes


@functools.lru_cache(maxsize=None)
def build(name):
    shape = SHAPE_BY_NAME[name]
    cap, L = shape.kp_cap, shape.slice_len
    rng = np.random.default_rng(20240 + cap)
    sizes = _frame_pair_sizes(cap)
    nfp = len(sizes) + 1                      # + the extremes pair
    desc = rng.integers(0, 256, (2 * nfp, cap, 32), dtype=np.uint8)
    counts = np.zeros(2 * nfp, np.int32)
    plants = []
    for k, (nq, nt) in enumerate(sizes):
        counts[2 * k], counts[2 * k + 1] = nq, nt
        q, t = desc[2 * k], desc[2 * k + 1]
        zq = int(rng.integers(0, nq)) if nq > 0 else -1
        if nq > 0:
            # an all-zero query: a train row past the count that is read as zeros would be at distance 0
            q[zq] = 0
        plants += _plant_frame_pair(rng, k, q, t, nq, nt, L, shape.slices > 1, zq)
    # extremes: 193 identical trains (four stages, the last with one live row) against their complement, a copy and
    # a copy with one bit flipped
    k = len(sizes)
    nq, nt = 65, 193
    counts[2 * k], counts[2 * k + 1] = nq, nt
    q, t = desc[2 * k], desc[2 * k + 1]
    x = t[0].copy()
    t[:nt] = x
    for qi, (cls, mask, d) in zip(rng.permutation(nq)[:3], (("complement", np.full(32, 255, np.uint8), 256),
                                                             ("identical", np.zeros(32, np.uint8), 0),
                                                             ("one_bit", flips(rng, 1), 1))):
        q[qi] = x ^ mask
        plants.append(Plant(2 * k, 2 * k + 1, int(qi), cls, "extremes", 0, 1, -1, (d, 0, d)))
    # poison: rows past a frame's count are copies of the partner frame's live rows
    live = desc.copy()
    for f in range(2 * nfp):
        n, m = int(counts[f]), int(counts[f ^ 1])
        if n < cap and m > 0:
            desc[f, n:] = live[f ^ 1, np.arange(cap - n) % m]
    # distinct (query frame, train frame) combinations: every partner pair (these hold counts[q] == 0 and
    # counts[t] == 0), frames against themselves, and cross pairs of any two frames
    combos = [(2 * k, 2 * k + 1) for k in range(nfp)]
    size_of = {sz: k for k, sz in reversed(list(enumerate(sizes)))}
    for f in (0, 1, 2 * nfp - 1, 2 * size_of[(cap, 0)] + 1, 2 * size_of[(cap - 1, 1)] + 1, 2 * size_of[(cap, 193)]):
        combos.append((f, f))
    while len(combos) < nfp + 6 + 12:
        a, b = (int(v) for v in rng.integers(0, 2 * nfp, 2))
        if (a, b) not in combos:
            combos.append((a, b))
    assert len(combos) <= shape.npairs
    combo_of_pair = rng.permutation(shape.npairs) % len(combos)
    qf = np.array([combos[c][0] for c in combo_of_pair], np.int32)
    tf = np.array([combos[c][1] for c in combo_of_pair], np.int32)
    for a in (desc, counts, qf, tf, combo_of_pair):
        a.setflags(write=False)
    return Case(shape, desc, counts, qf, tf, tuple(combos), combo_of_pair, tuple(plants))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per distinct combination: (best, idx, second) int32 arrays of counts[q] entries.  Computed once per shape
    and shared; read-only."""
    case = build(name)
    out = []
    for qfr, tfr in case.combos:
        r = top2_numpy(case.desc[qfr, :case.counts[qfr]], case.desc[tfr, :case.counts[tfr]])
        r = tuple(np.asarray(v).astype(np.int32) for v in r)
        for v in r:
            v.setflags(write=False)
        out.append(r)
    return tuple(out)


def plant_index(case):
    """{(qframe, tframe, query row): Plant} for failure messages."""
    return {(p.qframe, p.tframe, p.qi): p for p in case.plants}
