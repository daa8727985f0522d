"""GPU parity of both SearchByBoW forms (k_topk and the host replay, csrc/matcher.hip) with tests/bow_ref.py on the
planted cases of tests/bow_cases.py: one call per case, every case again with side 2's candidate lists reversed (the
expected answer recomputed by the reference), and all cases stacked as the keyframes of one batch call.
tests/test_bow_cases.py checks on the CPU that the cases realise the decisions they are named for."""
import numpy as np
import pytest

import bow_cases as bc

pytestmark = pytest.mark.gpu


def _items(c):
    return sorted({p.item for p in c.plants} | set(c.rot.items if c.rot else ()))


def _run(orbgpu_mod, form, c):
    m = orbgpu_mod.ORBmatcher(c.nnratio, True)
    if form == "kf_f":
        return m.SearchByBoW_KF_F(c.desc1, c.angle1, c.mp1, c.fv1, c.desc2, c.angle2, c.fv2)
    return m.SearchByBoW_KF_KF(c.desc1, c.angle1, c.mp1, c.fv1, c.desc2, c.angle2, c.mp2, c.fv2)


@pytest.mark.parametrize("order", ("as_built", "reversed"))
@pytest.mark.parametrize("form", ("kf_f", "kf_kf"))
def test_planted_cases_match_reference(orbgpu_mod, form, order):
    bad = []
    for name in bc.CASES:
        c = bc.cases()[name] if order == "as_built" else bc.reversed_lists(bc.cases()[name])
        want_n, want, _ = bc.expected(form, c)
        n, got = _run(orbgpu_mod, form, c)
        if n != want_n or not np.array_equal(got, want):
            diff = np.flatnonzero(got != want)[:8].tolist()
            bad.append((name, _items(c), n, want_n, diff, got[diff].tolist(), want[diff].tolist()))
    assert not bad, bad


@pytest.mark.parametrize("form", ("kf_f", "kf_kf"))
def test_cases_stacked_as_one_batch(orbgpu_mod, form):
    """Cases with the same ratio go into one batch call (the ratio is the call's)."""
    bad = []
    for ratio in sorted({bc.cases()[n].nnratio for n in bc.CASES}):
        names = [n for n in bc.CASES if bc.cases()[n].nnratio == ratio]
        shared, parts = bc.stacked(form, names)
        m = orbgpu_mod.ORBmatcher(ratio, True)
        kfs = [dict(desc=p["desc"], angle=p["angle"], mp=p["mp"], featvec=p["featvec"]) for p in parts]
        if form == "kf_f":
            res = m.SearchByBoW_KF_F_batch(kfs, shared[0], shared[1], shared[3])
        else:
            res = m.SearchByBoW_KF_KF_batch(shared[0], shared[1], shared[2], shared[3], kfs)
        assert len(res) == len(names)
        for name, p, (n, got) in zip(names, parts, res):
            want_n, want, _ = bc.expected(form, bc.cases()[name])
            full = np.full(len(shared[0]), -1, np.int32)
            full[p["offset"]:p["offset"] + p["n"]] = want
            if n != want_n or not np.array_equal(got, full):
                bad.append((name, _items(bc.cases()[name]), n, want_n, np.flatnonzero(got != full)[:8].tolist()))
    assert not bad, bad
