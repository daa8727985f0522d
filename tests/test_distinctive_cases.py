"""CPU checks of tests/distinctive_cases.py: the sort-based reference equals the oracle on every set, every census
item is planted and realised in the reference's row medians, and each set's hand-written winner and medians equal
what the reference computes."""
import numpy as np

import distinctive_cases as dc


def test_reference_equals_oracle(oracle_mod):
    for name, d in dc.sets().items():
        assert dc.distinctive(d.desc)[0] == oracle_mod.distinctive_descriptor(d.desc), name


def test_planted_outcomes_equal_the_reference():
    for name, d in dc.sets().items():
        idx, median, med = dc.distinctive(d.desc)
        assert (idx, median) == (d.winner, d.median), (name, idx, median)
        assert len(d.row_medians) == len(med) == len(d.desc)
        for i, want in enumerate(d.row_medians):
            assert want is None or med[i] == want, (name, i, med[i], want)


def test_census():
    seen = {}
    for name, d in dc.sets().items():
        idx, median, med = dc.distinctive(d.desc)
        n = len(d.desc)
        for item in d.items:
            ctx = (name, item)
            kind, _, v = item.rpartition("_")
            if kind == "win_bin":
                assert median == int(v) and med[idx] == int(v), ctx
                assert n == 1 or len(np.unique(d.desc, axis=0)) >= 2 or int(v) == 0, ctx
            elif kind == "row_bin":
                assert int(v) in med and median < int(v), ctx          # a losing row's median
            elif kind == "n":
                assert n == int(v), ctx
            elif item == "all_identical":
                assert len(np.unique(d.desc, axis=0)) == 1 and n > 64 and set(med) == {0}, ctx
            elif item == "tie_first_and_later_row":
                tied = [i for i, m in enumerate(med) if m == median]
                assert len(tied) >= 2 and tied[0] == idx > 0, ctx
            elif item == "winner_not_first_row":
                assert idx > 0 and med[0] > median, ctx
            elif item == "winner_beyond_lane_stride":
                assert idx >= 64 and [i for i, m in enumerate(med) if m == median] == [idx], ctx
            else:
                raise AssertionError(ctx)
            seen.setdefault(item, []).append(name)
        if any(it.startswith("win_bin") for it in d.items) and median > 0:
            assert len(np.unique(d.desc, axis=0)) >= 3, name       # clusters, not one noisy prototype
    for item, names in dc.BATCHES.items():
        full = [x for x in names if x is not None]
        assert all(x in dc.sets() for x in full)
        if item.startswith("nmp_"):
            assert len(names) == int(item[4:]) == len(full)
        else:
            inner = names[1:-1]
            assert None in inner and names[0] is not None and any(x is not None for x in inner)
            assert any(a is None and b is None for a, b in zip(names, names[1:]))      # two empties in a row too
        seen.setdefault(item, []).append(item)
    missing = [it for it in dc.ITEMS if it not in seen]
    assert not missing, missing
    assert set(seen) == set(dc.ITEMS)
    assert max(len(d.desc) for d in dc.sets().values()) <= 129
