"""GPU parity of ComputeDistinctiveDescriptors (k_distinctive, csrc/distinctive.hip) with the sort-based reference of
tests/distinctive_cases.py on its planted sets: each set alone, and the batches that leave waves of a block idle or
put map points without observations between full ones.  tests/test_distinctive_cases.py checks on the CPU that the
sets realise the histogram bins and sizes they are named for."""
import numpy as np
import pytest

import distinctive_cases as dc

pytestmark = pytest.mark.gpu


def _mismatches(got, names):
    bad = []
    for m, name in enumerate(names):
        want = -1 if name is None else dc.distinctive(dc.sets()[name].desc)[0]
        if got[m] != want:
            bad.append((m, name, dc.sets()[name].items if name else ("empty",), int(got[m]), want))
    return bad


def test_each_set_alone(orbgpu_mod):
    m = orbgpu_mod.ORBmatcher(0.6, True)
    bad = []
    for name, d in dc.sets().items():
        bad += _mismatches(m.ComputeDistinctiveDescriptors([d.desc]), [name])
    assert not bad, bad


@pytest.mark.parametrize("batch", sorted(dc.BATCHES))
def test_batches(orbgpu_mod, batch):
    names = dc.BATCHES[batch]
    m = orbgpu_mod.ORBmatcher(0.6, True)
    got = m.ComputeDistinctiveDescriptors([dc.EMPTY if n is None else dc.sets()[n].desc for n in names])
    bad = _mismatches(got, names)
    assert not bad, (batch, bad)
    # the same map points in the opposite order: every set lands on another wave
    got = m.ComputeDistinctiveDescriptors([dc.EMPTY if n is None else dc.sets()[n].desc for n in names[::-1]])
    bad = _mismatches(got, names[::-1])
    assert not bad, (batch, "reversed", bad)


def test_all_sets_in_one_call(orbgpu_mod):
    names = list(dc.sets())
    got = orbgpu_mod.ORBmatcher(0.6, True).ComputeDistinctiveDescriptors([dc.sets()[n].desc for n in names])
    bad = _mismatches(got, names)
    assert not bad, bad
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
