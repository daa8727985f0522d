"""CPU checks of tests/triangulation_cases.py: the restated SearchForTriangulation (tests/triangulation_ref.py) and
the oracle agree on every case, with bOnlyStereo off and on and with the candidate lists reversed; every census item
is planted and realised in the reference trace with the named operands; every plant's expected bestIdx2 equals the
trace."""
import numpy as np
import pytest

import triangulation_cases as tc
import triangulation_ref as ref


def _oracle(oracle_mod, c, only_stereo):
    fv1, k1 = oracle_mod.make_featvec(sorted(c.fv1), [c.fv1[k] for k in sorted(c.fv1)])
    fv2, k2 = oracle_mod.make_featvec(sorted(c.fv2), [c.fv2[k] for k in sorted(c.fv2)])
    return oracle_mod.search_for_triangulation(True, only_stereo, c.desc1, c.kps1, c.mp1, c.ur1, fv1, c.desc2, c.kps2,
                                               c.mp2, c.ur2, fv2, tc.F12.reshape(9), tc.EX, tc.EY, tc.SCALE2, tc.SIGMA2)


@pytest.mark.parametrize("only_stereo", (False, True))
@pytest.mark.parametrize("name", tc.CASES)
def test_reference_equals_oracle(oracle_mod, name, only_stereo):
    for c in (tc.cases()[name], tc.reversed_lists(tc.cases()[name])):
        pairs, _ = tc.expected(c, only_stereo)
        got = _oracle(oracle_mod, c, only_stereo)
        assert np.array_equal(pairs, got), (name, only_stereo, pairs.tolist(), got.tolist())


def test_operands_are_exact_in_float():
    """Integers below 2^20 everywhere the line and the gate read, so fused and unfused forms agree bit for bit."""
    for c in tc.cases().values():
        for k in (c.kps1, c.kps2):
            for f in ("x", "y"):
                assert (k[f] == np.round(k[f])).all() and (np.abs(k[f]) < 1024).all()
    assert (tc.F12 == np.round(tc.F12)).all() and np.abs(tc.F12).max() < 1024
    assert (100 * tc.SCALE2.astype(np.float64) == (np.float32(100) * tc.SCALE2)).all()


def test_census():
    seen = {}
    for name in tc.CASES:
        c = tc.cases()[name]
        tr = {s: tc.expected(c, s)[1] for s in (False, True)}
        vis = {s: {v["idx1"]: v for v in tr[s]["visits"]} for s in (False, True)}
        fillers = set(c.fillers)              # random descriptors: above TH_LOW from every query of their node
        for node, lst in c.fv2.items():
            for t in lst:
                if t in fillers:
                    for q in c.fv1.get(node, ()):
                        assert ref.descriptor_distance(c.desc1[q], c.desc2[t]) > 80, (name, node, q, t)
        for p in c.plants:
            for s, want in ((False, p.best), (True, p.best_stereo)):
                if want is not None:
                    assert vis[s][p.idx1]["best"] == want, (name, p, s, vis[s][p.idx1])
            v = vis[False][p.idx1]
            why = {x["idx2"]: x for x in v["cands"]}
            kept = [x for x in v["cands"] if x["why"] == "kept"]
            ctx, it = (name, p), p.item
            if it in ("tie_last_wins_across_lanes", "tie_beyond_64"):
                lst = c.fv2[v["node"]]
                pos = [lst.index(x["idx2"]) for x in kept]
                assert len(kept) == 2 and kept[0]["dist"] == kept[1]["dist"] and v["best"] == kept[1]["idx2"], ctx
                assert pos[1] - pos[0] > 64 and pos[0] % 64 != pos[1] % 64, ctx
            elif it == "tie_within_one_stride_pass":
                lst = c.fv2[v["node"]]
                pos = [lst.index(x["idx2"]) for x in kept]
                assert len(kept) == 2 and kept[0]["dist"] == kept[1]["dist"] and v["best"] == kept[1]["idx2"], ctx
                assert len(lst) <= 64 and pos[0] != pos[1], ctx
            elif it == "candidates_above_64":
                assert len(c.fv2[v["node"]]) > 64, ctx
            elif it == "dist_50":
                assert kept[0]["dist"] == 50 == v["best_dist"], ctx
            elif it == "dist_51":
                assert [x["why"] for x in v["cands"]] == ["dist"] and v["cands"][0]["dist"] == 51, ctx
            elif it.startswith("epipole_equal"):
                assert kept[0]["e2"] == kept[0]["lim"] and c.kps2[kept[0]["idx2"]]["octave"] == int(it[-1]), ctx
            elif it.startswith("epipole_inside"):
                x = v["cands"][0]
                assert x["why"] == "epipole" and x["lim"] - x["e2"] <= 15 and c.kps2[x["idx2"]]["octave"] == int(it[-1]), ctx
            elif it.startswith("epipole_gate_skipped"):
                k2 = c.kps2[kept[0]["idx2"]]
                assert kept[0]["e2"] is None and (tc.EX - k2["x"]) ** 2 + (tc.EY - k2["y"]) ** 2 < 100, ctx
                assert (c.ur1[p.idx1] >= 0) != (c.ur2[kept[0]["idx2"]] >= 0), ctx
                assert (c.ur1[p.idx1] >= 0) == it.endswith("1"), ctx
            elif it.startswith("dsqr_"):
                x = v["cands"][0]
                lv = int(it[-1])
                lim = 3.84 * float(tc.SIGMA2[lv])
                assert c.kps2[x["idx2"]]["octave"] == lv and x["den"] == 25, ctx
                assert x["why"] == ("kept" if "below" in it else "line"), ctx
                assert (float(x["dsqr"]) < lim) == ("below" in it) and 0.15 < abs(float(x["dsqr"]) - lim) < 0.8, ctx
            elif it == "den_zero":
                assert [x["why"] for x in v["cands"]] == ["den"] and v["cands"][0]["den"] == 0, ctx
            elif it.startswith("closer_candidate_fails"):
                whys = [x["why"] for x in v["cands"]]
                assert whys == ["kept", "line" if it.endswith("line") else "epipole", "kept"], ctx
                d = [x["dist"] for x in v["cands"]]
                assert d[1] < d[2] < d[0] and v["best_dist"] == d[2], ctx
            elif it == "only_stereo_train_mono":
                assert c.ur2[p.best] < 0 <= c.ur2[p.best_stereo] and vis[True][p.idx1]["cands"][0]["why"] == "stereo", ctx
            elif it == "only_stereo_query_mono":
                assert vis[True][p.idx1]["outcome"] == ref.MONO and v["outcome"] == ref.MATCHED, ctx
            elif it == "train_has_map_point":
                assert v["cands"][0]["why"] == "mp" and (c.desc2[v["cands"][0]["idx2"]] == c.desc1[p.idx1]).all(), ctx
            elif it == "query_has_map_point":
                assert v["outcome"] == ref.HAS_MP and vis[True][p.idx1]["outcome"] == ref.HAS_MP, ctx
            elif it == "train_matched_twice":
                assert sum(w["best"] == p.best for w in tr[False]["visits"]) == 2, ctx
            elif it == "culled_pair_removed":
                pairs = tc.expected(c, False)[0]
                assert p.idx1 not in pairs[:, 0].tolist() and v["bin"] not in tr[False]["ind"], ctx
            else:
                raise AssertionError(ctx)
            seen.setdefault(it, []).append(name)
        if c.rot is not None:
            t = tr[False]
            assert tuple(t["sizes"]) == c.rot.sizes and t["ind"] == c.rot.ind and t["culled"] == c.rot.culled
            s, ind = c.rot.sizes, c.rot.ind
            for it in c.rot.items:
                if it == "rot_negative_wrap":
                    assert any(w["bin"] == 12 and c.kps1[w["idx1"]]["angle"] < c.kps2[w["best"]]["angle"]
                               for w in t["visits"])
                elif it == "rot_bin_30_to_0":
                    assert any(w["bin"] == 0 and c.kps1[w["idx1"]]["angle"] == 900 for w in t["visits"])
                elif it == "rot_round_half":
                    assert any(w["bin"] == 1 and c.kps1[w["idx1"]]["angle"] == 15 and c.kps2[w["best"]]["angle"] == 0
                               for w in t["visits"])
                elif it == "maxima_first_second_tied":
                    assert s[ind[0]] == s[ind[1]] and ind[0] < ind[1]
                elif it == "maxima_third_tied_first_wins":
                    assert [i for i, x in enumerate(s) if x == s[ind[2]]][0] == ind[2] and s.count(s[ind[2]]) == 2
                elif it == "maxima_third_at_cutoff_kept":
                    assert np.float32(s[ind[2]]) == np.float32(0.1) * np.float32(s[ind[0]])
                else:
                    raise AssertionError(it)
                seen.setdefault(it, []).append(name)
        else:
            assert tr[False]["culled"] == tr[True]["culled"] == 0
    missing = [it for it in tc.ITEMS if it not in seen]
    assert not missing, missing
    assert set(seen) == set(tc.ITEMS)
