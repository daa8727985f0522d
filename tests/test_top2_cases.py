"""The planted top-2 cases (tests/top2_cases.py) through the reference alone, and the launch-shape table against
the library's slice arithmetic (orb_hamming_top2_slices, host only).  No GPU."""
import collections

import numpy as np
import pytest

import top2_cases as tc

NAMES = [s.name for s in tc.SHAPES]


@pytest.mark.parametrize("name", NAMES)
def test_every_plant_realises_its_triple(name):
    """The reference returns the planted (best, index, second) for every planted query of every class and
    position: the random background never interferes (planted distances <= 40), no plant is left out."""
    case, ref = tc.build(name), tc.reference(name)
    combo = {cb: i for i, cb in enumerate(case.combos)}
    assert len(case.plants) > 300
    for p in case.plants:
        best, idx, second = ref[combo[(p.qframe, p.tframe)]]
        got = (int(best[p.qi]), int(idx[p.qi]), int(second[p.qi]))
        assert got == p.expect, (name, p)
        assert max(p.expect[0], p.expect[2]) <= 40 or p.pos == "extremes", p
        assert p.a < p.b < case.counts[p.tframe] and p.c < case.counts[p.tframe] and p.qi < case.counts[p.qframe], p
    # no train row serves two plants of a frame
    rows = collections.Counter((p.tframe, r) for p in case.plants if p.pos != "extremes"
                               for r in (p.a, p.b, p.c) if r >= 0)
    assert max(rows.values()) == 1


@pytest.mark.parametrize("name", NAMES)
def test_every_position_pair_is_present(name):
    case = tc.build(name)
    shape, L = case.shape, case.shape.slice_len
    have = collections.Counter((p.cls, p.pos) for p in case.plants)
    for pos in tc.POSITIONS:
        if pos in tc.SLICED_ONLY and shape.slices == 1:
            continue
        for cls in tc.VARIANTS:
            assert have[(cls, pos)] >= 1, (name, cls, pos)
    for cls in ("complement", "identical", "one_bit"):
        assert have[(cls, "extremes")] == 1, (name, cls)
    # the positions are what their names say
    stage, tile, half = (lambda r: r // tc.STAGE), (lambda r: r // tc.TILE), (lambda r: r >> 2 & 1)
    for p in case.plants:
        a, b, nt = p.a, p.b, int(case.counts[p.tframe])
        if p.pos == "b_last":
            assert b == nt - 1
        elif p.pos == "slice_boundary":
            assert b % L == 0 and a == b - 1
        elif p.pos == "first_last_stage":
            assert stage(a) == 0 and stage(b) == stage(nt - 1) > 0 and nt % tc.STAGE
        elif p.pos == "tile0_tile1":
            assert a % tc.STAGE == 31 and b == a + 1
        elif p.pos == "adjacent_stages":
            assert a % tc.STAGE == 63 and b == a + 1 and a // L == b // L
        elif p.pos == "stage_j_j2":
            assert stage(b) == stage(a) + 2 and (L < 3 * tc.STAGE or a // L == b // L)
        elif p.pos == "first_last_slice":
            assert a // L == 0 and b // L == (nt - 1) // L > 0
        elif p.pos == "same_tile_other_half":
            assert tile(a) == tile(b) and b == a ^ 4
        elif p.pos == "same_tile_same_half":
            assert tile(a) == tile(b) and half(a) == half(b)
    # a tie whose later row has the smaller row-in-tile bits (the strict-less rule on dist alone decides it)
    assert any(p.cls == "tie" and tile(p.a) != tile(p.b) and p.b % tc.TILE < p.a % tc.TILE for p in case.plants)
    # exact copies of a query in two different stages
    assert any(p.cls == "copies" and stage(p.a) != stage(p.b) for p in case.plants)
    # a best in the last, cut-short stage of every train count that has one; a second from another slice
    cut = {int(case.counts[p.tframe]) for p in case.plants if p.pos == "b_last"}
    assert cut >= {n for n in tc.frame_counts(shape.kp_cap) if n >= 2}, (name, sorted(cut))
    if shape.slices > 1:
        assert any(p.cls in ("later_better", "earlier_better") and p.a // L != p.b // L for p in case.plants)


@pytest.mark.parametrize("name", NAMES)
def test_counts_pairs_and_poison(name):
    case = tc.build(name)
    shape, cap = case.shape, case.shape.kp_cap
    counts = case.counts
    assert case.desc.shape == (len(counts), cap, 32) and case.desc.nbytes < 3 << 20
    want = set(tc.frame_counts(cap))
    assert set(counts[1::2].tolist()) == want and set(counts[0::2].tolist()) <= want
    assert len(case.qf) == len(case.tf) == shape.npairs
    assert {(int(q), int(t)) for q, t in zip(case.qf, case.tf)} == set(case.combos)   # every combination is launched
    assert len(set(case.combos)) == len(case.combos)
    assert any(q == t for q, t in case.combos) and any(q != t and q != t ^ 1 for q, t in case.combos)
    assert any(counts[q] == 0 and counts[t] > 0 for q, t in case.combos)
    assert any(counts[t] == 0 and counts[q] > 0 for q, t in case.combos)
    assert any(counts[t] == 1 and counts[q] > 0 for q, t in case.combos)
    # every query frame holds an all-zero query (a train row past the count read as zeros would be at distance 0)
    for f in range(0, len(counts), 2):
        if counts[f] > 0 and not any(p.pos == "extremes" and p.qframe == f for p in case.plants):
            assert (case.desc[f, :counts[f]].max(1) == 0).any(), f
    # rows past the count are exact copies of the partner's live rows: distance 0 to it if ever read
    for f in range(len(counts)):
        n, m = int(counts[f]), int(counts[f ^ 1])
        if n < cap and m > 0:
            assert np.array_equal(case.desc[f, n:], case.desc[f ^ 1, np.arange(cap - n) % m]), f
            best, _, _ = tc.top2_numpy(case.desc[f ^ 1, :min(m, cap - n)], case.desc[f, n:])
            assert (best == 0).all(), f


def test_reference_sentinels_and_multiplicity():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    best, idx, second = tc.top2_numpy(q, q[:0])
    assert (best == 257).all() and (idx == -1).all() and (second == 257).all() and len(best) == 5
    best, idx, second = tc.top2_numpy(q, q[2:3])
    assert best[2] == 0 and (idx == 0).all() and (second == 257).all()
    assert all(len(v) == 0 for v in tc.top2_numpy(q[:0], q))
    # against a bit-by-bit count; two trains at the best distance: second == best, the first index wins
    t = np.concatenate([q[3:4] ^ tc.flips(rng, 9), q[3:4] ^ tc.flips(rng, 9), q[3:4] ^ tc.flips(rng, 11), q])
    best, idx, second = tc.top2_numpy(q, t)
    D = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(2)
    assert np.array_equal(best, D.min(1)) and np.array_equal(idx, D.argmin(1))
    assert np.array_equal(second, np.sort(D, 1)[:, 1])
    assert (best[3], idx[3], second[3]) == (0, 6, 9) and (best == 0).all()
    best, idx, second = tc.top2_numpy(q[3:4], t[:3])
    assert (best[0], idx[0], second[0]) == (9, 0, 9)
    for d in (0, 1, 40, 256):
        assert int(np.unpackbits(tc.flips(rng, d)).sum()) == d


@pytest.mark.parametrize("name", NAMES)
def test_shape_table_against_the_library(name, orbgpu_mod):
    """The launch shapes are derived from top2_batch_slices / top2_slice_len as they stand.  The library must cut
    each shape into the slices the table expects, and those slices must be long enough for the stage loop to run:
    with ceil(kp_cap / 64) >= (min_stages - 1) * slices + 1 whole stages to cover, some slice has at least
    min_stages of them (three where the table wants an LDS buffer reused, i.e. >= 2 * slices + 1; two for the
    448-row shape, whose 128-row slices give one loop iteration each).  A heuristic that falls back to one-stage
    slices fails here."""
    from orbgpu import _lib
    s = tc.SHAPE_BY_NAME[name]
    L = _lib.lib()
    assert L.orb_hamming_top2_slices(s.npairs, s.kp_cap, s.kp_cap) == s.slices, name
    nstages = -(-s.kp_cap // tc.STAGE)
    assert nstages >= (s.min_stages - 1) * s.slices + 1, name
    # slices are whole stages: the slice length is the one multiple of 64 that covers kp_cap in `slices` slices
    fits = [n for n in range(tc.STAGE, s.kp_cap + tc.STAGE, tc.STAGE) if -(-s.kp_cap // n) == s.slices]
    assert fits == [s.slice_len] or (s.slices == 1 and fits[0] == s.slice_len), (name, fits)
    assert s.slice_len >= s.min_stages * tc.STAGE


def test_shape_table_pinned():
    assert [(s.kp_cap, s.npairs, s.slices, s.slice_len) for s in tc.SHAPES] == [(330, 1024, 1, 384),
                                                                               (640, 300, 3, 256),
                                                                               (448, 171, 4, 128)]
    assert [s.min_stages for s in tc.SHAPES] == [3, 3, 2]
    assert (3 * 3 * 300) % 8 != 0   # the XCD remap's remainder path
