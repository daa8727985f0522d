"""GPU parity of SearchForTriangulation (k_triangulation and its host staging, csrc/matcher.hip) with
tests/triangulation_ref.py on the planted cases of tests/triangulation_cases.py: the single call and the batch, with
bOnlyStereo off and on, and every case again with KF2's candidate lists reversed (the kernel keeps the last candidate
of a tie; the expected answer is recomputed by the reference).  tests/test_triangulation_cases.py checks on the CPU
that the cases realise the decisions they are named for."""
import numpy as np
import pytest

import triangulation_cases as tc

pytestmark = pytest.mark.gpu


def _items(c):
    return sorted({p.item for p in c.plants} | set(c.rot.items if c.rot else ()))


def _variants():
    for name in tc.CASES:
        yield name, "as_built", tc.cases()[name]
        yield name, "reversed", tc.reversed_lists(tc.cases()[name])


@pytest.mark.parametrize("only_stereo", (False, True))
def test_planted_cases_match_reference(orbgpu_mod, only_stereo):
    m = orbgpu_mod.ORBmatcher(0.6, True)
    bad = []
    for name, order, c in _variants():
        want, _ = tc.expected(c, only_stereo)
        got = m.SearchForTriangulation(c.desc1, c.kps1, c.mp1, c.ur1, c.fv1, c.desc2, c.kps2, c.mp2, c.ur2, c.fv2,
                                       tc.F12, tc.EX, tc.EY, tc.SCALE2, tc.SIGMA2, bOnlyStereo=only_stereo)
        if not np.array_equal(got, want):
            bad.append((name, order, _items(c), got.tolist(), want.tolist()))
    assert not bad, bad


@pytest.mark.parametrize("only_stereo", (False, True))
def test_batch_matches_reference(orbgpu_mod, only_stereo):
    """KF1 against its KF2 as built and reversed in one orb_search_for_triangulation_batch call."""
    m = orbgpu_mod.ORBmatcher(0.6, True)
    bad = []
    for name in tc.CASES:
        c = tc.cases()[name]
        both = (c, tc.reversed_lists(c))
        others = [dict(desc2=v.desc2, kps2=v.kps2, has_mp2=v.mp2, uright2=v.ur2, featvec2=v.fv2, F12=tc.F12, ex=tc.EX,
                       ey=tc.EY, scale_factors2=tc.SCALE2, level_sigma2_2=tc.SIGMA2) for v in both]
        res = m.SearchForTriangulationBatch(c.desc1, c.kps1, c.mp1, c.ur1, c.fv1, others, bOnlyStereo=only_stereo)
        assert len(res) == 2
        for v, got, order in zip(both, res, ("as_built", "reversed")):
            want, _ = tc.expected(v, only_stereo)
            if not np.array_equal(got, want):
                bad.append((name, order, _items(c), got.tolist(), want.tolist()))
    assert not bad, bad
