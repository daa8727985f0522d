"""Both SearchByBoW forms between resident frames (orb_search_by_bow_frames_kf_f / _kf_kf: k_bow_items, k_topk over the
train handle's own arrays, the host replay) against the host-pointer entry points and tests/bow_ref.py, exactly, on the
planted cases of tests/bow_cases.py as built and with side 2's lists reversed, and a KF-F batch of three keyframes.
The case "edges" holds topk_list_exhausted_by_taken, whose query is decided only after a re-rank on the resident
items; the planted expectation pins it."""
import numpy as np
import pytest

import bow_cases as bc

pytestmark = pytest.mark.gpu
BOUNDS = (0.0, 640.0, 0.0, 480.0)


def _frame(orbgpu, m, desc, angle, fv):
    k = np.zeros(len(desc), orbgpu.KP_DTYPE)
    k["x"], k["y"], k["angle"] = 100.0, 100.0, np.asarray(angle, np.float32)
    F = orbgpu.Frame(m, desc, k, bounds=BOUNDS)
    F.set_featvec(fv, m)
    return F


def _variants():
    for name in bc.CASES:
        yield name, "as_built", bc.cases()[name]
        yield name, "reversed", bc.reversed_lists(bc.cases()[name])


@pytest.mark.parametrize("form", ("kf_f", "kf_kf"))
def test_planted_cases(orbgpu_mod, form):
    bad = []
    for name, order, c in _variants():
        m = orbgpu_mod.ORBmatcher(c.nnratio, True)
        F1, F2 = _frame(orbgpu_mod, m, c.desc1, c.angle1, c.fv1), _frame(orbgpu_mod, m, c.desc2, c.angle2, c.fv2)
        try:
            if form == "kf_f":
                (n, got), = m.SearchByBoW_Frames_KF_F([dict(frame=F1, mp=c.mp1)], F2)
                hn, host = m.SearchByBoW_KF_F(c.desc1, c.angle1, c.mp1, c.fv1, c.desc2, c.angle2, c.fv2)
            else:
                n, got = m.SearchByBoW_Frames_KF_KF(F1, c.mp1, F2, c.mp2)
                hn, host = m.SearchByBoW_KF_KF(c.desc1, c.angle1, c.mp1, c.fv1, c.desc2, c.angle2, c.mp2, c.fv2)
        finally:
            F1.close()
            F2.close()
        want_n, want, _ = bc.expected(form, c)
        if (n, hn) != (want_n, want_n) or not np.array_equal(got, want) or not np.array_equal(host, want):
            bad.append((name, order, n, hn, want_n, np.flatnonzero(got != want)[:8].tolist()))
    assert not bad, bad


def test_rerank_case_is_realised(orbgpu_mod):
    """topk_list_exhausted_by_taken through the resident KF-F form: the query's match is the planted one."""
    c = bc.cases()["edges"]
    plant, = [p for p in c.plants if p.item == "topk_list_exhausted_by_taken"]
    m = orbgpu_mod.ORBmatcher(c.nnratio, True)
    F1, F2 = _frame(orbgpu_mod, m, c.desc1, c.angle1, c.fv1), _frame(orbgpu_mod, m, c.desc2, c.angle2, c.fv2)
    try:
        (n, got), = m.SearchByBoW_Frames_KF_F([dict(frame=F1, mp=c.mp1)], F2)
    finally:
        F1.close()
        F2.close()
    assert plant.exp_kf_f[0] == bc.A and got[plant.exp_kf_f[3]] == plant.idx1


def test_kf_f_batch_of_three(orbgpu_mod):
    """edges, disjoint (no common node) and edges again with every mp flag 0, against one Frame that holds the side 2
    of all three (bow_cases.stacked moves indices and node ids apart)."""
    names = ["edges", "disjoint", "edges"]
    shared, parts = bc.stacked("kf_f", names)
    parts[2] = dict(parts[2], mp=np.zeros_like(parts[2]["mp"]))
    m = orbgpu_mod.ORBmatcher(0.5, True)
    kfs = [dict(desc=p["desc"], angle=p["angle"], mp=p["mp"], featvec=p["featvec"]) for p in parts]
    want = m.SearchByBoW_KF_F_batch(kfs, shared[0], shared[1], shared[3])
    Ff = _frame(orbgpu_mod, m, shared[0], shared[1], shared[3])
    Fk = [_frame(orbgpu_mod, m, p["desc"], p["angle"], p["featvec"]) for p in parts]
    try:
        got = m.SearchByBoW_Frames_KF_F([dict(frame=F, mp=p["mp"]) for F, p in zip(Fk, parts)], Ff)
    finally:
        Ff.close()
        for F in Fk:
            F.close()
    assert len(got) == len(want) == 3
    for (n, a), (wn, w) in zip(got, want):
        assert n == wn and np.array_equal(a, w)
    assert want[0][0] > 5 and want[1][0] == 0 and want[2][0] == 0
