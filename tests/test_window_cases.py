"""CPU checks of tests/window_cases.py: the restated window matchers and grid lookup (tests/window_ref.py) agree with
the oracle (candidate lists and matches, level0_only on and off, lists as built and reversed); every census item is
planted and realised in the reference trace; every plant's hand-written outcome equals the trace."""
import numpy as np
import pytest

import window_cases as wc
import window_ref as ref


def test_grid_lookup_equals_oracle(oracle_mod):
    c = wc.case()
    lists = wc.candidates()
    for i1, k in enumerate(c.kps1):
        got = oracle_mod.features_in_area(c.kps2, *wc.BOUNDS, float(k["x"]), float(k["y"]), wc.R, int(k["octave"]),
                                          int(k["octave"]))
        assert got.tolist() == list(lists[i1]), i1


@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("level0_only", (True, False))
def test_reference_equals_oracle(oracle_mod, level0_only, reverse):
    c = wc.case()
    n, m, _ = wc.expected(level0_only, reverse)
    off, idx = wc.csr(wc.candidates(reverse))
    on, om = oracle_mod.window_match(wc.NNRATIO, True, level0_only, c.desc1, c.kps1, c.desc2, c.kps2, off, idx)
    assert n == on and np.array_equal(m, om), (n, on, np.flatnonzero(m != om)[:8])
    assert n == (m >= 0).sum()


def test_census():
    c = wc.case()
    lists = wc.candidates()
    res = {True: wc.expected(True), False: wc.expected(False)}
    # integers everywhere the grid lookup reads; regions do not see each other; fillers are far from their queries
    for k in (c.kps1, c.kps2):
        assert (k["x"] == np.round(k["x"])).all() and (k["y"] == np.round(k["y"])).all()
    fillers = set(c.fillers)
    for i1, lst in enumerate(lists):
        for t in lst:
            assert c.region2[t] == c.region1[i1], (i1, t)
            if t in fillers:
                assert ref.descriptor_distance(c.desc1[i1], c.desc2[t]) > 80, (i1, t)
    assert res[True][2]["culled"] == res[False][2]["culled"] == 0
    seen = {}
    for p in c.plants:
        for mode, exp in ((True, p.init), (False, p.window)):
            v = res[mode][2]["visits"][p.i1]
            assert v["i1"] == p.i1
            if exp is not None:
                assert (v["outcome"], v["d1"], v["d2"], v["best"]) == exp, (p, mode, v)
            if p.final is not None:
                assert res[mode][1][p.i1] == p.final, (p, mode)
        v = res[True][2]["visits"][p.i1]
        lst, it = list(lists[p.i1]), p.item
        dist = [ref.descriptor_distance(c.desc1[p.i1], c.desc2[t]) for t in lst]
        if it.startswith("th_low_"):
            assert v["d1"] == int(it[7:]), p
        elif it == "ratio_equal":
            assert v["d1"] == wc.NNRATIO * v["d2"], p
        elif it == "ratio_below":
            assert v["d1"] + 1 == wc.NNRATIO * v["d2"], p
        elif it == "one_candidate":
            assert len(lst) == 1 and v["d2"] == ref.INT_MAX, p
        elif it == "second_best_ties_best":
            assert dist.count(v["d1"]) == 2 and v["d1"] == v["d2"] == min(dist) and len(lst) <= 64, p
        elif it == "second_best_ties_best_beyond_64":
            pos = [k for k, d in enumerate(dist) if d == v["d1"]]
            assert len(pos) == 2 and pos[1] - pos[0] > 64 and pos[0] % 64 != pos[1] % 64 and v["d1"] == v["d2"], p
        elif it == "earlier_match_replaced":
            later = [w for w in res[True][2]["visits"] if w["replaced"] == p.i1]
            assert len(later) == 1 and later[0]["i1"] > p.i1 and later[0]["d1"] < v["d1"] and later[0]["best"] == v["best"], p
            assert res[True][1][p.i1] == -1 and v["outcome"] == ref.ACCEPTED
        elif it == "later_better_match_replaces":
            assert v["replaced"] >= 0 and v["replaced"] < p.i1 and res[True][1][v["replaced"]] == -1, p
        elif it == "blocked_at_equal_distance":
            assert any(d == md for _, d, md in v["blocked"]) and v["outcome"] == ref.ACCEPTED, p
        elif it == "level0_only_query_skipped":
            assert c.kps1[p.i1]["octave"] == 1 and res[True][1][p.i1] == -1 and res[False][1][p.i1] == p.window[3], p
        elif it == "candidate_on_another_level":
            same = np.flatnonzero((c.desc2 == c.desc1[p.i1]).all(1))
            assert len(same) == 1 and c.kps2[same[0]]["octave"] != c.kps1[p.i1]["octave"] and same[0] not in lst, p
            assert abs(c.kps2[same[0]]["x"] - c.kps1[p.i1]["x"]) < wc.R
        elif it == "empty_window":
            assert lst == [] and 0 <= c.kps1[p.i1]["x"] < 512, p
        elif it == "window_off_the_grid":
            assert lst == [] and (c.kps1[p.i1]["x"] - wc.R) / 8 >= ref.COLS, p
        elif it in ("rect_edge_equal_excluded", "rect_edge_one_inside"):
            same = np.flatnonzero((c.desc2 == c.desc1[p.i1]).all(1))
            dx = np.abs(c.kps2["x"][same] - c.kps1["x"][p.i1])
            dy = np.abs(c.kps2["y"][same] - c.kps1["y"][p.i1])
            assert len(same) == 5 and (np.maximum(dx, dy) == wc.R).all() and not set(same) & set(lst), p
            assert {(16.0, 0.0), (0.0, 16.0), (16.0, 16.0)} <= set(zip(dx.tolist(), dy.tolist()))
            k = c.kps2[v["best"]]
            assert abs(k["x"] - c.kps1["x"][p.i1]) == wc.R - 1 == abs(k["y"] - c.kps1["y"][p.i1]) and lst == [v["best"]], p
        elif it == "candidates_above_64":
            assert 64 < len(lst) <= 128, p
        elif it == "best_beyond_lane_stride":
            assert lst.index(v["best"]) >= 64, (p, lst.index(v["best"]))
        elif it == "topk_list_exhausted_by_matched_distance":
            order = np.argsort(dist, kind="stable")
            blocked = {t for t, _, _ in v["blocked"]}
            assert {lst[k] for k in order[:8]} == blocked and lst[order[8]] == v["best"], p
            assert len(lst) - len(blocked) > 8 and dist[order[10]] > 80, p
        else:
            raise AssertionError(p)
        seen.setdefault(it, []).append(p.i1)
    missing = [it for it in wc.ITEMS if it not in seen]
    assert not missing, missing
    assert set(seen) == set(wc.ITEMS)
    assert len(c.desc1) <= 300 and len(c.desc2) <= 300
