"""CPU checks of tests/bow_cases.py: the restated SearchByBoW loops (tests/bow_ref.py) and the oracle agree on every
case in both forms, with the candidate lists as built and reversed, and stacked as a batch; every census item
(bow_cases.ITEMS) is planted and realised in the reference trace; every plant's hand-written outcome equals the
trace."""
import numpy as np
import pytest

import bow_cases as bc
import bow_ref as ref

FORMS = ("kf_f", "kf_kf")


def _oracle(oracle_mod, form, c):
    fv1, k1 = oracle_mod.make_featvec(sorted(c.fv1), [c.fv1[k] for k in sorted(c.fv1)])
    fv2, k2 = oracle_mod.make_featvec(sorted(c.fv2), [c.fv2[k] for k in sorted(c.fv2)])
    if form == "kf_f":
        return oracle_mod.search_by_bow_kf_f(c.nnratio, True, c.desc1, c.angle1, c.mp1, fv1, c.desc2, c.angle2, fv2)
    return oracle_mod.search_by_bow_kf_kf(c.nnratio, True, c.desc1, c.angle1, c.mp1, fv1, c.desc2, c.angle2, c.mp2, fv2)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", bc.CASES)
def test_reference_equals_oracle(oracle_mod, name, form):
    for c in (bc.cases()[name], bc.reversed_lists(bc.cases()[name])):
        n, m, _ = bc.expected(form, c)
        on, om = _oracle(oracle_mod, form, c)
        assert n == on and np.array_equal(m, om), (name, form, n, on, np.flatnonzero(m != om)[:8])
        assert n == (m >= 0).sum()


@pytest.mark.parametrize("form", FORMS)
def test_stacked_batch_is_the_cases_side_by_side(form):
    """What the GPU batch test relies on: against the stacked shared side each keyframe finds exactly its own case's
    matches, moved by the case's offset."""
    shared, parts = bc.stacked(form, bc.CASES)
    for name, p in zip(bc.CASES, parts):
        c = bc.cases()[name]
        n, m, _ = bc.expected(form, c)
        if form == "kf_f":
            sn, sm, _ = ref.search_by_bow(form, c.nnratio, True, p["desc"], p["angle"], p["mp"], p["featvec"],
                                          shared[0], shared[1], shared[2], shared[3])
            own = sm[p["offset"]:p["offset"] + p["n"]]
            assert sn == n and np.array_equal(own, m) and (sm >= 0).sum() == n, name
        else:
            sn, sm, _ = ref.search_by_bow(form, c.nnratio, True, shared[0], shared[1], shared[2], shared[3],
                                          p["desc"], p["angle"], p["mp"], p["featvec"])
            own = sm[p["offset"]:p["offset"] + p["n"]]
            assert sn == n and np.array_equal(own, m) and (sm >= 0).sum() == n, name


def test_census():
    seen = {}
    for name in bc.CASES:
        c = bc.cases()[name]
        traces = {f: bc.expected(f, c) for f in FORMS}
        # every random filler stays more than 80 bits from every query of its node (on either side of TH_LOW and of
        # every planted second best nothing but planted partners decides)
        fillers = set(c.fillers)
        for node, lst in c.fv2.items():
            for t in lst:
                if t in fillers:
                    for q in c.fv1.get(node, ()):
                        assert ref.descriptor_distance(c.desc1[q], c.desc2[t]) > 80, (name, node, q, t)
        for form in FORMS:
            n, m, tr = traces[form]
            by_idx1 = {}
            for v in tr["visits"]:
                assert v["idx1"] not in by_idx1
                by_idx1[v["idx1"]] = v
            for p in c.plants:
                exp = p.exp_kf_f if form == "kf_f" else p.exp_kf_kf
                if exp is None:
                    continue
                v = by_idx1[p.idx1]
                assert (v["outcome"], v["d1"], v["d2"], v["best"]) == exp, (name, form, p, v)
        tf, tk = traces["kf_f"][2], traces["kf_kf"][2]
        vf = {v["idx1"]: v for v in tf["visits"]}
        for p in c.plants:
            ctx, it = (name, p), p.item
            if it.startswith("th_low_"):
                assert vf[p.idx1]["d1"] == int(it[7:]), ctx
            elif it == "ratio_equal":
                v = vf[p.idx1]
                assert v["d1"] == c.nnratio * v["d2"] and v["outcome"] == ref.RATIO, ctx
            elif it == "ratio_below":
                v = vf[p.idx1]
                assert v["d1"] + 1 == c.nnratio * v["d2"] and v["outcome"] == ref.ACCEPTED, ctx
            elif it == "ratio_float_0p6_30_50":
                assert c.nnratio == 0.6 and vf[p.idx1]["d2"] == 50 and vf[p.idx1]["d1"] in (30, 31), ctx
                assert np.float32(30) < np.float32(0.6) * np.float32(50) and not 30 < 0.6 * 50
            elif it == "second_best_ties_best_across_lanes":
                v = vf[p.idx1]
                lst = c.fv2[v["node"]]
                pos = [k for k, t in enumerate(lst) if ref.descriptor_distance(c.desc1[p.idx1], c.desc2[t]) == v["d1"]]
                assert v["d1"] == v["d2"] and len(pos) == 2 and pos[1] - pos[0] > 64 and pos[0] % 64 != pos[1] % 64, ctx
                assert lst[pos[0]] == v["best"]
            elif it == "one_candidate":
                assert vf[p.idx1]["d2"] == 256 and vf[p.idx1]["seen"] == 1, ctx
            elif it == "kf_map_point_missing_or_bad":
                assert not c.mp1[p.idx1] and (c.desc2 == c.desc1[p.idx1]).all(1).any(), ctx
                assert (traces["kf_f"][1] != p.idx1).all() and traces["kf_kf"][1][p.idx1] == -1
            elif it == "train_map_point_missing_or_bad":
                assert not c.mp2[p.exp_kf_f[3]] and p.exp_kf_kf[3] != p.exp_kf_f[3], ctx
            elif it in ("taken_within_node", "taken_across_nodes"):
                v = vf[p.idx1]
                d = [ref.descriptor_distance(c.desc1[p.idx1], c.desc2[t]) for t in c.fv2[v["node"]]]
                taken = c.fv2[v["node"]][int(np.argmin(d))]
                if taken != v["best"]:          # the later query: its nearest went to an earlier one
                    first = next(w for w in tf["visits"] if w["best"] == taken and w["outcome"] == ref.ACCEPTED)
                    assert tf["visits"].index(first) < tf["visits"].index(v), ctx
                    assert (first["node"] == v["node"]) == (it == "taken_within_node"), ctx
                    seen.setdefault(it + ":loser", []).append(name)
            elif it == "decoy_in_another_node":
                assert p.idx1 not in vf and (c.desc2 == c.desc1[p.idx1]).all(1).any(), ctx
            elif it == "lower_bound_skip_side1":
                assert tf["skips"][0] >= 1 and min(c.fv1) < min(c.fv2), ctx
            elif it == "lower_bound_skip_side2":
                assert tf["skips"][1] >= 1 and min(c.fv2) not in c.fv1, ctx
            elif it == "lower_bound_skips_two_nodes":
                k1 = sorted(c.fv1)
                gap = [a for a, b in zip(k1, k1[1:]) if a not in c.fv2 and b not in c.fv2]
                assert gap and any(k > gap[0] for k in tf["nodes"]), ctx
            elif it == "lower_bound_runs_off_the_end":
                assert max(c.fv1) not in tf["nodes"] and max(c.fv2) > max(c.fv1) > max(tf["nodes"]), ctx
            elif it == "node_above_64_candidates":
                assert 64 < len(c.fv2[vf[p.idx1]["node"]]) <= 128, ctx
            elif it == "node_above_512_candidates":
                assert 512 < len(c.fv2[vf[p.idx1]["node"]]) <= 600, ctx
            elif it == "best_beyond_lane_stride":
                assert c.fv2[vf[p.idx1]["node"]].index(vf[p.idx1]["best"]) >= 512, ctx
            elif it == "topk_list_exhausted_by_taken":
                v = vf[p.idx1]
                lst = c.fv2[v["node"]]
                d = np.array([ref.descriptor_distance(c.desc1[p.idx1], c.desc2[t]) for t in lst])
                order = np.argsort(d, kind="stable")
                taken = {w["best"] for w in tf["visits"][:tf["visits"].index(v)] if w["outcome"] == ref.ACCEPTED}
                assert all(lst[k] in taken for k in order[:8]) and lst[order[8]] == v["best"], ctx
                assert v["seen"] == len(lst) - 8 > 8 and v["outcome"] == ref.ACCEPTED, ctx
                assert d[order[10]] > 80                      # the fillers are far
            elif it == "no_common_node":
                assert tf["nodes"] == [] and traces["kf_f"][0] == traces["kf_kf"][0] == 0, ctx
            else:
                raise AssertionError(ctx)
            seen.setdefault(it, []).append(name)
        if c.rot is not None:
            for form in FORMS:
                n, m, tr = traces[form]
                assert tuple(tr["sizes"]) == c.rot.sizes and tr["ind"] == c.rot.ind and tr["culled"] == c.rot.culled, \
                    (name, form, tr["sizes"], tr["ind"], tr["culled"])
                assert n == sum(c.rot.sizes) - c.rot.culled == (m >= 0).sum()
            vis, s, ind = tf["visits"], c.rot.sizes, c.rot.ind
            for it in c.rot.items:
                ctx = (name, it)
                if it == "rot_negative_wrap":
                    assert any(c.angle1[v["idx1"]] < c.angle2[v["best"]] and v["bin"] == 12 for v in vis), ctx
                elif it == "rot_bin_30_to_0":
                    assert any(ref.c_round(v["rotf"]) == 30 and v["bin"] == 0 for v in vis), ctx
                elif it == "rot_round_half":
                    assert any(v["rotf"] == np.float32(0.5) and v["bin"] == 1 for v in vis), ctx
                elif it == "maxima_first_second_tied":
                    assert s[ind[0]] == s[ind[1]] and ind[0] < ind[1], ctx
                elif it == "maxima_third_tied_first_wins":
                    tied = [i for i, x in enumerate(s) if x == s[ind[2]]]
                    assert len(tied) == 2 and tied[0] == ind[2], ctx
                elif it == "maxima_third_at_cutoff_kept":
                    assert np.float32(s[ind[2]]) == np.float32(0.1) * np.float32(s[ind[0]]), ctx
                elif it == "maxima_third_below_cutoff":
                    assert ind[2] == -1 and ind[1] >= 0 and sorted(s)[-3] > 0, ctx
                elif it == "maxima_second_below_cutoff":
                    assert ind[1] == ind[2] == -1 and sorted(s)[-2] > 0, ctx
                else:
                    raise AssertionError(ctx)
                seen.setdefault(it, []).append(name)
        else:
            for form in FORMS:       # the edge cases keep the histogram out of the way
                assert traces[form][2]["culled"] == 0, (name, form)
    assert "taken_within_node:loser" in seen and "taken_across_nodes:loser" in seen
    missing = [it for it in bc.ITEMS if it not in seen]
    assert not missing, missing
    assert {k for k in seen if ":" not in k} == set(bc.ITEMS)
    for c in bc.cases().values():
        assert len(c.desc1) <= 300 and len(c.desc2) <= 800 and max(len(v) for v in c.fv2.values()) <= 600
