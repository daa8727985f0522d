"""GPU parity of SearchByMatchBird in both forms (orb_search_by_match_bird: k_projection_topk over the birdview grid
+ match_bird_replay; orb_search_by_match_bird_frame: orb_window_match_grid's path + the carry-over) against
tests/match_bird_ref.py, the restated loops of ORBmatcher.cc:1901-1921 and :2000-2114: the result vector and nmatches
equal exactly.  The inputs come from tests/match_bird_cases.py; each case also asserts, from the restatement's own
counters, that it reaches the branches it is for."""
import numpy as np
import pytest

import match_bird_cases as mc
import match_bird_ref as ref

pytestmark = pytest.mark.gpu


def _same(name, got, want):
    (n, m), (want_m, want_n) = got, want
    bad = np.flatnonzero(m != want_m)[:8]
    assert n == want_n and bad.size == 0 and len(m) == len(want_m), \
        (name, n, want_n, bad.tolist(), m[bad].tolist(), want_m[bad].tolist())


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_matches_reference(orbgpu_mod, oracle_mod, name):
    want_m, want_n, counters = mc.expected(oracle_mod, name)
    zero = [k for k in mc.WANT[name] if counters[k] == 0]
    assert not zero, (name, zero)
    _same(name, mc.run_product(orbgpu_mod, mc.case(name)), (want_m, want_n))


def test_exhausted_list_is_reranked(orbgpu_mod, oracle_mod):
    """Fourteen identical queries on a window of twenty: the ninth finds the eight entries of its list held at their
    distance with twelve more in the window (a list of mc.TOPK entries cannot decide it: the product re-ranks)."""
    c = mc.case("kf_exhaustion")
    want_m, want_n, counters = mc.expected(oracle_mod, "kf_exhaustion")
    assert counters["exhausted_queries"] >= 14 - mc.TOPK
    rep = c["kf"]["index"][(c["kf"]["x"] == 40) & (c["kf"]["y"] == 40)]
    assert len(rep) == 14 and np.isin(rep, want_m).sum() > mc.TOPK   # more of them matched than one list holds
    _same("kf_exhaustion", mc.run_product(orbgpu_mod, c), (want_m, want_n))


@pytest.mark.parametrize("check_ori", [False, True])
def test_check_ori_both_ways(orbgpu_mod, oracle_mod, check_ori):
    c = dict(mc.case("kf_r10_ori"), check_ori=check_ori)
    want_m, want_n, counters = mc.reference(oracle_mod, c)
    assert (counters["culled_entries"] > 0) == check_ori and ((want_m == -2).any() == check_ori)
    _same("kf_r10_ori", mc.run_product(orbgpu_mod, c), (want_m, want_n))


def test_second_best_at_256_is_kept(orbgpu_mod, oracle_mod):
    """nnratio 0.3: a second best at 256 rejects bests of 77..100 that a list cut at 256 would accept."""
    c = mc.case("kf_second_at_256")
    want_m, want_n, _ = mc.expected(oracle_mod, "kf_second_at_256")
    n, m = mc.run_product(orbgpu_mod, c)
    _same("kf_second_at_256", (n, m), (want_m, want_n))
    assert n == 12        # the bests of 60..76 only; with the cut every best <= 100 would be accepted (28)


def test_max_dist_and_nnratio_are_the_callers(orbgpu_mod, oracle_mod):
    c = mc.case("kf_r15")
    for md, nnratio in ((30, 0.7), (256, 0.7), (100, 0.2), (100, 1.0)):
        cc = dict(c, max_dist=md, nnratio=nnratio)
        want_m, want_n, _ = mc.reference(oracle_mod, cc)
        _same((md, nnratio), mc.run_product(orbgpu_mod, cc), (want_m, want_n))


def test_edges(orbgpu_mod, oracle_mod):
    c = mc.case("kf_r20_th60")
    q, f = c["kf"], c["frame"]
    nt = len(f["kps"])
    none = {k: v[:0] for k, v in q.items()}
    n, m = mc.run_product(orbgpu_mod, dict(c, kf=none))                          # no queries
    assert n == 0 and len(m) == nt and (m == -1).all()
    empty = dict(desc=f["desc"][:0], kps=f["kps"][:0], bounds=f["bounds"])
    n, m = mc.run_product(orbgpu_mod, dict(c, frame=empty))                      # no trains
    assert n == 0 and len(m) == 0
    n, m = mc.run_product(orbgpu_mod, dict(c, r=0.0))                            # |dx| < 0 never holds
    assert n == 0 and (m == -1).all()
    for x, y in ((-500.0, 100.0), (100.0, 5000.0), (1e30, -1e30)):               # windows entirely off the grid
        far = dict(q, x=np.full_like(q["x"], x), y=np.full_like(q["y"], y))
        n, m = mc.run_product(orbgpu_mod, dict(c, kf=far))
        assert n == 0 and (m == -1).all()
    n, m = mc.run_product(orbgpu_mod, dict(c, max_dist=0))                       # only exact descriptors
    want_m, want_n, _ = mc.reference(oracle_mod, dict(c, max_dist=0))
    _same("max_dist 0", (n, m), (want_m, want_n))
    # the frame form without keypoints on either side
    fc = mc.case("frame_w15_all")
    nothing = dict(desc=fc["cur"]["desc"][:0], kps=fc["cur"]["kps"][:0], bounds=fc["cur"]["bounds"])
    n, m = mc.run_product(orbgpu_mod, dict(fc, cur=nothing))
    assert n == 0 and len(m) == 0
    n, m = mc.run_product(orbgpu_mod, dict(fc, last=nothing, has_mp=np.zeros(0, np.uint8)))
    assert n == 0 and len(m) == len(fc["cur"]["kps"]) and (m == -1).all()


def test_frame_form_is_birdview_match_plus_carry_over(orbgpu_mod, oracle_mod):
    """match_cur is the inverse of orb_window_match_grid's vnMatches12 restricted to has_mp_last."""
    c = mc.case("frame_w20_mixed")
    cur, last = c["cur"], c["last"]
    grid = orbgpu_mod.frame_grid(cur["kps"], *cur["bounds"])
    m = orbgpu_mod.ORBmatcher(c["nnratio"], c["check_ori"])
    n12, m12 = m.window_match_grid(False, last["desc"], last["kps"], cur["desc"], cur["kps"], grid, c["window"])
    want_m, want_n, without = ref.carry_over(m12, c["has_mp"], len(cur["kps"]))
    assert n12 == want_n + without
    _same("carry", mc.run_product(orbgpu_mod, c), (want_m, want_n))


def test_argument_errors_with_a_context(orbgpu_mod, oracle_mod):
    c = mc.case("kf_borders")
    bad_x = c["kf"]["x"].copy()
    bad_x[5] = np.nan
    for kw in (dict(max_dist=257), dict(max_dist=-1), dict(r=-0.5), dict(r=float("nan")), dict(r=float("inf")),
               dict(pt_x=bad_x)):
        with pytest.raises(orbgpu_mod.OrbError) as e:
            mc.run_product(orbgpu_mod, c, **kw)
        assert e.value.status == -1, kw
    inv_w, inv_h, off, idx = orbgpu_mod.frame_grid(c["frame"]["kps"], *c["frame"]["bounds"])
    bad_idx = idx.copy()
    bad_idx[3] = len(c["frame"]["kps"])
    with pytest.raises(orbgpu_mod.OrbError) as e:
        mc.run_product(orbgpu_mod, c, grid_bird=(inv_w, inv_h, off, bad_idx))
    assert e.value.status == -1
    n, m = mc.run_product(orbgpu_mod, c)      # the context still works after the refusals
    assert n == mc.expected(oracle_mod, "kf_borders")[1]
