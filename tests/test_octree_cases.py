"""CPU: the planted octree cases of tests/octree_cases.py are what they claim to be.  For every case the oracle's
level-0 candidates are exactly the planted stamps (positions, responses, vToDistributeKeys order), tests/octree_ref.py
on them gives the oracle's level-0 keypoints in order under both tie policies, every census item a case is there for
is found in the reference trace, and the cases together realise the whole census.  tests/test_gpu_octree_cases.py
runs the same cases through k_octree."""
import time

import numpy as np
import pytest

import octree_cases as oc

CASES = oc.cases()


def _oracle(oracle_mod, case, flags=0):
    o = oracle_mod.OracleExtractor(case.N, 1.2, 1, oc.INI_TH, oc.MIN_TH, flags)
    assert o.run(case.frame.image()) >= 0
    return o


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_is_what_it_claims(oracle_mod, case):
    t = time.perf_counter()
    cands, (o0, t0), (o1, t1), items = oc.solved(case)
    took = time.perf_counter() - t
    assert took < 5, ("the Python reference must stay quick", case.name, took)
    print(case.name, len(cands), "candidates;", [(r["phase"], r["before"], r["after"]) for r in t0["rounds"]])
    for it in sorted(items):
        print("   ", it)
    for flags, out in ((0, o0), (oracle_mod.TIE_REVERSE_SEQ, o1)):
        o = _oracle(oracle_mod, case, flags)
        assert np.array_equal(o.candidates(0), cands), (case.name, "the oracle's candidates are not the planted stamps")
        k = o.level_keypoints(0)
        got = np.stack([k["x"], k["y"], k["response"]], 1).astype(np.int32).reshape(-1, 3)
        want = np.array(out, np.int32).reshape(-1, 3) + np.array([oc.BORDER, oc.BORDER, 0], np.int32)
        assert np.array_equal(got, want), (case.name, flags, "octree_ref differs from the oracle", len(got), len(want))
    missing = [it for it in case.items if it not in items]
    assert not missing, (case.name, "census items not realised", missing)
    if any(it in oc.TIE_ITEMS for it in case.items):
        assert o0 != o1, (case.name, "the two tie policies give the same output")


def test_the_cases_realise_the_whole_census():
    have = {}
    for c in CASES:
        assert all(it in oc.CENSUS for it in c.items), c.name
        for it in oc.solved(c)[3]:
            have.setdefault(it, []).append(c.name)
    for it in oc.CENSUS:
        print(f"{it}: {', '.join(have.get(it, [])) or 'MISSING'}")
    assert not [it for it in oc.CENSUS if it not in have]
    claimed = {it for c in CASES for it in c.items}
    assert not [it for it in oc.CENSUS if it not in claimed], "every census item is some case's stated purpose"


def test_the_large_case_is_large():
    """The list after the fast-forward's last round (6) holds more than 2,048 nodes, two-key ones among those at
    positions >= 2,048 and one-key ones too; 2,517 stamps do not fit the 1,336 keys of LDS left at N = 2,400."""
    case = next(c for c in CASES if c.name == "big-N2400")
    cands, (_, t0), _, _ = oc.solved(case)
    r6 = t0["rounds"][5]
    assert r6["phase"] == 1 and oc.ff_depth(1, case.N) == 6 and 2048 < r6["after"] < case.N
    assert sum(p >= 2048 for p in r6["multi_pos"]) >= 8 and r6["after"] - 1 not in r6["multi_pos"]
    assert len(cands) >= 2300 and oc.lds_keys_single(case.N, case.geo) == 1336 < len(cands)
    assert oc.node_cap(2488, 1) * 64 + 160 <= 160 * 1024 < oc.node_cap(2489, 1) * 64 + 160
