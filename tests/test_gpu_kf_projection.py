"""GPU: orb_project_best_batch (k_projection_best) against the restatement and orb_project_best_host, the five
wrappers of the keyframe searches against the restated loops, the edges, and the replay rule with the batched search
on the GPU."""
import ctypes

import numpy as np
import pytest

import kf_projection_cases as cases
import kf_projection_ref as ref
from test_kf_projection_ref import _host_all, _host_search, _target, check_replay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(orbgpu_mod):
    return orbgpu_mod.ORBmatcher(0.9, True)


def _lists(out):
    return [(a.tolist(), b.tolist()) for a, b in out]


@pytest.mark.parametrize("gate", [0, 1])
def test_batch_equals_restatement_and_host(orbgpu_mod, oracle_mod, matcher, gate):
    targets = cases.fuse_targets()
    ts = [_target(orbgpu_mod, kf, pts) for kf, pts in targets]
    want = [cases.expected_fuse(oracle_mod, k, gate == 1)[:2] for k in range(len(targets))]
    host = [_host_all(orbgpu_mod, gate, kf, pts) for kf, pts in targets]
    assert _lists(host) == _lists(want)
    assert _lists(matcher.project_best_batch(gate, ts[:3])) == _lists(want[:3])        # the three in one call
    for k in range(3):                                                                  # each alone
        assert _lists(matcher.project_best_batch(gate, [ts[k]])) == _lists(want[k:k + 1]), k
    # targets without queries and without trains in the middle of a batch
    order = [0, 3, 1, 4, 2]
    assert _lists(matcher.project_best_batch(gate, [ts[k] for k in order])) == _lists([want[k] for k in order])
    assert want[4][0].tolist() == [-1] * 20 and want[4][1].tolist() == [-1] * 20


def test_wrappers_fuse_and_sim3(orbgpu_mod, oracle_mod, matcher):
    targets = cases.fuse_targets()
    pk = [(cases.product_kf(orbgpu_mod, kf), pts) for kf, pts in targets]
    for chi2, fn in ((True, matcher.Fuse), (False, matcher.Fuse_Scw)):
        want = [cases.expected_fuse(oracle_mod, k, chi2)[:2] for k in range(len(targets))]
        assert _lists(fn(pk)) == _lists(want)
    kf1, kf2, p12, p21 = cases.sim3_case()
    nfound, vn, _ = cases.expected(oracle_mod, "sim3")
    got_n, got = matcher.SearchBySim3(cases.product_kf(orbgpu_mod, kf1), cases.product_kf(orbgpu_mod, kf2), p12, p21)
    assert got_n == nfound and got.tolist() == vn.tolist()


def test_wrappers_keyframe_search_by_projection(orbgpu_mod, oracle_mod):
    pts, kf, taken = cases.loop_case()
    match, n, _ = cases.expected(oracle_mod, "loop")
    got_n, got = orbgpu_mod.ORBmatcher(0.75, True).SearchByProjection_KF_Scw(pts, cases.product_kf(orbgpu_mod, kf), taken)
    assert got_n == n and got.tolist() == match.tolist()
    pts, kf, taken, orb_dist, ori = cases.reloc_case()
    match, n, _ = cases.expected(oracle_mod, "reloc")
    got_n, got = orbgpu_mod.ORBmatcher(0.75, ori).SearchByProjection_F_KF(pts, cases.product_kf(orbgpu_mod, kf), taken,
                                                                        orb_dist)
    assert got_n == n and got.tolist() == match.tolist()


def test_edges(orbgpu_mod, oracle_mod, matcher):
    from orbgpu import _lib
    assert matcher.project_best_batch(0, []) == []
    kf, pts = cases.fuse_targets()[1]
    t = _target(orbgpu_mod, kf, pts)
    # every window outside the grid
    out = dict(t, q=t["q"].copy())
    out["q"]["u"], out["q"]["v"] = -500.0, 2000.0
    bi, bd = matcher.project_best_batch(1, [out])[0]
    assert (bi == -1).all() and (bd == -1).all()
    # r = 0: `fabs(dx) < r` admits nothing
    zero = dict(t, q=t["q"].copy())
    zero["q"]["r"] = 0.0
    zero["q"]["u"][:50], zero["q"]["v"][:50] = kf["kps"]["x"][:50], kf["kps"]["y"][:50]
    bi, bd = matcher.project_best_batch(0, [zero])[0]
    assert (bi == -1).all() and (bd == -1).all()
    assert all(orbgpu_mod.project_best_host(0, zero, i) == (-1, -1) for i in range(50))
    # a refused call writes nothing and leaves the context working
    bad = dict(t, q=t["q"].copy())
    bad["q"]["u"][3] = np.nan
    with pytest.raises(orbgpu_mod.OrbError, match="target 1: query window not finite"):
        matcher.project_best_batch(1, [t, bad])
    want = cases.expected_fuse(oracle_mod, 1, True)
    bi, bd = matcher.project_best_batch(1, [t])[0]
    assert bi.tolist() == want[0].tolist() and bd.tolist() == want[1].tolist()
    assert _lib.lib().orb_project_best_batch(matcher._ctx.h, 0, 0, None) == 0


@pytest.mark.parametrize("scw", [False, True])
def test_replay_rule_with_the_batched_search_on_the_gpu(orbgpu_mod, matcher, scw):
    gate = 0 if scw else 1

    def batch(targets):
        return matcher.project_best_batch(gate, [_target(orbgpu_mod, kf, pts) for kf, pts, _ in targets])
    check_replay(batch, _host_search(orbgpu_mod, gate), scw)
