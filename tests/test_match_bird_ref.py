"""CPU: tests/match_bird_ref.py, the restated SearchByMatchBird (ORBmatcher.cc:1901-1921, :2000-2114), pinned by
hand-worked cases of a few points each (the expected vectors are written out), and tests/match_bird_cases.py checked
to reach the branches each case is for."""
import numpy as np
import pytest

import match_bird_cases as mc
import match_bird_ref as ref

f32 = np.float32
BOUNDS = (0.0, 384.0, 0.0, 384.0)


def D(n, skip=0):
    """A descriptor with bits [skip, skip + n) set: D(a) and D(b) are |a - b| apart, D(n) is n from D(0)."""
    d = np.zeros(32, np.uint8)
    for b in range(skip, skip + n):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def frame(trains):
    """trains: (x, y, octave, descriptor[, angle])"""
    from oracle import KP_DTYPE
    k = np.zeros(len(trains), KP_DTYPE)
    for i, t in enumerate(trains):
        k["x"][i], k["y"][i], k["octave"][i] = t[0], t[1], t[2]
        k["angle"][i] = t[4] if len(t) > 4 else 0.0
    return dict(desc=np.stack([t[3] for t in trains]), kps=k, bounds=BOUNDS)


def keyframe(points):
    """points: (k, x, y, descriptor[, angle])"""
    return dict(index=np.array([p[0] for p in points], np.int32), x=np.array([p[1] for p in points], f32),
                y=np.array([p[2] for p in points], f32), desc=np.stack([p[3] for p in points]),
                angle=np.array([p[4] if len(p) > 4 else 0.0 for p in points], f32))


def run(oracle_mod, points, trains, nnratio, check_ori=False, r=10.0):
    m, n, c = ref.search_kf_f(oracle_mod, keyframe(points), frame(trains), r, nnratio, check_ori)
    return m.tolist(), n, c


def test_distance_helper(oracle_mod):
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    assert ref.descriptor_distance(a, b) == oracle_mod.descriptor_distance(a, b)
    assert ref.descriptor_distance(D(0), D(30)) == 30 and ref.descriptor_distance(D(25), D(40)) == 15
    assert ref.descriptor_distance(D(0), np.bitwise_not(D(0))) == 256


def test_a_single_candidate_is_accepted_without_a_second(oracle_mod):
    # bestLevel = 0, bestLevel2 = -1: the levels differ, the ratio is not looked at (nnratio 0 would reject all)
    m, n, _ = run(oracle_mod, [(7, 100, 100, D(0))], [(101, 99, 0, D(30)), (300, 300, 0, D(1))], 0.0)
    assert m == [7, -1] and n == 1


def test_b_ratio_only_between_equal_octaves(oracle_mod):
    trains = [(100, 100, 0, D(20)), (102, 101, 1, D(22)),      # different octaves: 20 is accepted against 22
              (300, 300, 1, D(20)), (302, 301, 1, D(22)),      # equal octaves: 20 < 0.6 * 22 fails
              (200, 50, 2, D(10)), (202, 51, 2, D(40))]        # equal octaves: 10 < 0.6 * 40 holds
    pts = [(3, 100, 100, D(0)), (5, 300, 300, D(0)), (8, 200, 50, D(0))]
    m, n, c = run(oracle_mod, pts, trains, 0.6)
    assert m == [3, -1, -1, -1, 8, -1] and n == 2 and c["different_level_accepts"] == 1


def test_c_second_best_at_256_rejects(oracle_mod):
    trains = [(100, 100, 0, D(80)), (101, 101, 0, np.bitwise_not(D(0)))]
    m, n, c = run(oracle_mod, [(0, 100, 100, D(0))], trains, 0.3)     # 80 < 256 * 0.3 = 76.8 fails
    assert m == [-1, -1] and n == 0 and c["seconds_at_256"] == 1
    # had the second best stayed at INT_MAX (a list cut at 256), the same query would be accepted:
    assert run(oracle_mod, [(0, 100, 100, D(0))], trains[:1], 0.3)[:2] == ([0], 1)
    assert f32(80) < f32(ref.INT_MAX) * f32(0.3)
    m, n, _ = run(oracle_mod, [(0, 100, 100, D(0))], trains, 0.35)    # 80 < 89.6
    assert m == [0, -1] and n == 1


def test_d_a_closer_later_query_steals_and_both_count(oracle_mod):
    trains = [(100, 100, 0, D(30)), (102, 100, 1, D(40))]
    pts = [(2, 100, 100, D(0)), (4, 101, 100, D(25))]      # k = 2 takes train 0 at 30; k = 4 reaches it at 5
    m, n, c = run(oracle_mod, pts, trains, 0.6)
    assert m == [4, -1] and n == 2 and c["steals"] == 1    # train 1 stays free: k = 2 does not fall back


def test_e_an_equal_distance_does_not_steal(oracle_mod):
    trains = [(100, 100, 0, D(30)), (102, 100, 1, D(40))]
    pts = [(2, 100, 100, D(0)), (4, 101, 100, D(0))]       # k = 4 is at 30 too: 30 <= 30 skips train 0
    m, n, c = run(oracle_mod, pts, trains, 0.6)
    assert m == [2, 4] and n == 2 and c["steals"] == 0 and c["le_skips"] == 1


def test_f_cull_counts_every_entry(oracle_mod):
    # train angles 0; a query angle of 30 b lands in bin b.  Bins 0, 1, 2 are kept (4, 2, 2 entries), bin 3 holds
    # train 7 twice (owner k = 20, then stolen by k = 21), bin 4 holds train 8 once (k = 22), which k = 23 steals
    # from bin 0.
    spots = [(40 * i + 20, 30) for i in range(9)]
    trains = [(x, y, 0, D(30)) for x, y in spots]
    ang = [0, 0, 0, 30, 30, 60, 60]
    pts = [(10 + i, spots[i][0], spots[i][1], D(0), ang[i]) for i in range(7)]
    pts += [(20, *spots[7], D(0), 90), (21, *spots[7], D(25), 90), (22, *spots[8], D(0), 120), (23, *spots[8], D(25), 0)]
    m, n, c = run(oracle_mod, pts, trains, 0.6, check_ori=True)
    # 11 acceptances, 3 culled entries: train 7 twice (nmatches drops by two for one train), train 8 once although
    # its last owner k = 23 sits in the kept bin 0
    assert m == [10, 11, 12, 13, 14, 15, 16, -2, -2] and n == 8
    assert c["steals"] == 2 and c["culled_entries"] == 3 and c["culled_entries_on_reset_or_reowned"] == 3
    m, n, _ = run(oracle_mod, pts, trains, 0.6, check_ori=False)
    assert m == [10, 11, 12, 13, 14, 15, 16, 21, 23] and n == 11


def test_g_frame_form_counts_only_points_with_a_map_point(oracle_mod):
    cur = frame([(300, 300, 0, D(12)), (200, 200, 1, D(7)), (100, 100, 0, D(3))])
    last = frame([(101, 99, 0, D(0)), (198, 201, 1, D(0)), (303, 301, 0, D(0))])
    m12, n12 = ref.birdview_match(oracle_mod, last, cur, 15, 0.9, True)
    assert m12.tolist() == [2, 1, 0] and n12 == 3
    m, n, c = ref.search_frame(oracle_mod, cur, last, 15, 0.9, True, np.array([1, 0, 1], np.uint8))
    assert m.tolist() == [2, -1, 0] and n == 2 and c == dict(birdview_matches=3, matched_without_map_point=1)
    m, n, _ = ref.search_frame(oracle_mod, cur, last, 15, 0.9, True, None)
    assert m.tolist() == [-1, -1, -1] and n == 0
    # BirdviewMatch looks on the query's own octave only (:1808): an octave apart nothing matches
    last["kps"]["octave"] = [1, 0, 1]
    assert ref.search_frame(oracle_mod, cur, last, 15, 0.9, True, np.ones(3, np.uint8))[1] == 0


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_cases_reach_their_branches(oracle_mod, name):
    c = mc.case(name)
    m, n, counters = mc.expected(oracle_mod, name)
    zero = [k for k in mc.WANT[name] if counters[k] == 0]
    assert not zero, (name, zero, counters)
    if c["form"] == "kf":
        assert 40 <= len(c["kf"]["index"]) <= 300
        assert 40 <= len(c["frame"]["kps"]) <= 300 and n > 0
    else:
        assert (n > 0) == (c["has_mp"] is not None and bool(c["has_mp"].any()))


def test_every_counter_is_reached_somewhere():
    assert {k for v in mc.WANT.values() for k in v} >= set(ref.COUNTERS)


def test_nmatches_is_not_the_number_of_owned_trains(oracle_mod):
    """Steals are counted twice, culled double entries twice: the return value and the vector disagree."""
    diff = {name: mc.expected(oracle_mod, name)[1] - int((mc.expected(oracle_mod, name)[0] >= 0).sum())
            for name in mc.CASES if mc.case(name)["form"] == "kf"}
    assert any(d > 0 for d in diff.values()), diff
