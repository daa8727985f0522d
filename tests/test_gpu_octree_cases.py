"""GPU: k_octree (csrc/extract_kernels.hip) on the planted cases of tests/octree_cases.py, against the plain Python
restatement of DistributeOctTree in tests/octree_ref.py.  For every case and both tie policies the level-0 candidates
equal the oracle's, the level-0 keypoints equal octree_ref's exactly and in order (integers, no tolerance), and the
extraction output equals the oracle's byte for byte: through ORBextractor's call, through a BatchExtractor holding
every frame that shares the case's size and N (per-kernel launches), and through the dataflow launch, which takes
batches of at most two frames (the octree body at 1,024 threads; its task stamps show that it ran).
Every context runs twice, so the second launch finds the first one's leftovers in the scratch buffers.
tests/test_octree_cases.py shows on the CPU that the cases realise the census; a failure here names the case and the
census items it carries."""
import numpy as np
import pytest

import octree_cases as oc

pytestmark = pytest.mark.gpu

CASES = oc.cases()
VARIANTS = (0, 1)      # pinned tie policy, ORB_VARIANT_TIE_REVERSE (== ORACLE_TIE_REVERSE_SEQ)


def _expected(oracle_mod, case, variant):
    cands, s0, s1, items = oc.solved(case)
    out = (s0, s1)[variant][0]
    want = np.array(out, np.int32).reshape(-1, 3) + np.array([oc.BORDER, oc.BORDER, 0], np.int32)
    o = oracle_mod.OracleExtractor(case.N, 1.2, 1, oc.INI_TH, oc.MIN_TH, variant)
    ok, od = o(case.frame.image())
    return o.candidates(0).copy(), want, ok, od, sorted(items)


def _check(where, case, variant, items, exp, cand, lvl, kps, desc):
    ocand, want, ok, od = exp
    tag = (where, case.name, "variant", variant, "census items:", items)
    assert np.array_equal(cand, ocand), tag + ("debug_candidates differ from the oracle", len(cand), len(ocand))
    if not np.array_equal(lvl, want):
        n = min(len(lvl), len(want))
        first = next((i for i in range(n) if not np.array_equal(lvl[i], want[i])), n)
        pytest.fail(str(tag + ("debug_level_keypoints differ from octree_ref", len(lvl), len(want), "first at", first,
                               lvl[first:first + 3].tolist(), want[first:first + 3].tolist())))
    assert len(kps) == len(ok) and kps.tobytes() == ok.tobytes() and np.array_equal(desc, od), \
        tag + ("the extraction output differs from the oracle",)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_single_frame_call(orbgpu_mod, oracle_mod, case, variant):
    *exp, items = _expected(oracle_mod, case, variant)
    g = orbgpu_mod.ORBextractor(case.N, 1.2, 1, oc.INI_TH, oc.MIN_TH, variant=variant)
    try:
        for rep in range(2):
            kps, desc = g(case.frame.image())
            _check(f"ORBextractor call {rep}", case, variant, items, exp, g.debug_candidates(0),
                   g.debug_level_keypoints(0), kps, desc)
    finally:
        g.close()


def _groups():
    """The frames that share a size and an N: one batch each (a BatchExtractor has one nfeatures)."""
    by = {}
    for c in CASES:
        by.setdefault((c.geo.w, c.N), [])
    for (w, n), lst in by.items():
        for f in oc.frames().values():
            if f.geo.w == w and (len(f.stamps) < 1000 or any(c.frame is f and c.N == n for c in CASES)):
                lst.append(oc.Case(f.name, n, ()))
    return by


GROUPS = _groups()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("key", sorted(GROUPS), ids=[f"{w}x240-N{n}" for w, n in sorted(GROUPS)])
def test_batch(orbgpu_mod, oracle_mod, monkeypatch, key, variant):
    """Every small frame of the size (and the large ones that have a case at this N) as one batch with this N, through
    the per-kernel launches (k_octree at 512 threads, one block per frame)."""
    group = GROUPS[key]
    w, n = key
    exps = [_expected(oracle_mod, c, variant) for c in group]
    monkeypatch.setenv("ORBGPU_FLOW", "0")   # read at orb_create
    e = orbgpu_mod.BatchExtractor(n, w, oc.H, len(group), nlevels=1, ini_th=oc.INI_TH, min_th=oc.MIN_TH, variant=variant)
    try:
        e.upload(np.stack([c.frame.image() for c in group]))
        for rep in range(2):
            e.launch()
            e.sync()
            for f, (c, (*exp, items)) in enumerate(zip(group, exps)):
                kps, desc = e.results(f)
                _check(f"batch of {len(group)}, frame {f}, launch {rep}", c, variant, items, exp,
                       e.debug_candidates(0, f), e.debug_level_keypoints(0, f), kps, desc)
    finally:
        e.close()


FLOW_OCTREE = 2      # the task kinds of the dataflow launch: resize, fast, octree, describe, chain (tools/flow_stamps.py)


def _flow_octree_done(orbgpu_mod, e, nframes):
    """The dataflow launch's per-task stamps (ORBGPU_FLOW_STAMPS=1: [ticket, wait over, done, kind | level << 8 |
    frame << 16 | workgroup << 32] per task; only k_extract_flow writes them, and the buffer exists only once a plan
    for this batch was built): when each frame's level-0 octree task ended."""
    st = np.zeros(1 << 16, np.uint64)
    n = orbgpu_mod._lib.lib().orb_debug_fast_stamps(e.h, st.ctypes.data, len(st))
    assert n > 0, "no dataflow plan was built for this batch: the per-kernel launches ran"
    st = st[:n - n % 4].reshape(-1, 4)
    done = {}
    for ticket, _, end, ident in st.tolist():
        if ticket and end and ident & 0xFFFF == FLOW_OCTREE and (ident >> 16) & 0xFFFF < nframes:
            done[(ident >> 16) & 0xFFFF] = end
    return done


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_dataflow_launch(orbgpu_mod, oracle_mod, monkeypatch, case, variant):
    """The dataflow launch takes batches of one or two frames: the case's frame and a small one of its size as a batch
    of two (the case in slot 0 under the pinned tie policy, in slot 1 under the reversed one), octree_task at 1,024
    threads (16 waves in the binned sort, 64 bytes less LDS for the keys).  The launch's own task stamps show that it
    was taken, in both launches of the context."""
    other = max((f for f in oc.frames().values() if f.geo.w == case.geo.w and f is not case.frame and len(f.stamps) < 1000),
                key=lambda f: len(f.stamps))
    pair = [case, oc.Case(other.name, case.N, ())]
    if variant:
        pair.reverse()
    exps = [_expected(oracle_mod, c, variant) for c in pair]
    monkeypatch.setenv("ORBGPU_FLOW", "1")          # read at orb_create
    monkeypatch.setenv("ORBGPU_FLOW_STAMPS", "1")
    monkeypatch.delenv("ORBGPU_FLOW_CHAIN", raising=False)
    monkeypatch.delenv("ORBGPU_FLOW_BLOCKS", raising=False)
    e = orbgpu_mod.BatchExtractor(case.N, case.geo.w, oc.H, 2, nlevels=1, ini_th=oc.INI_TH, min_th=oc.MIN_TH,
                                  variant=variant)
    try:
        e.upload(np.stack([c.frame.image() for c in pair]))
        before = {0: 0, 1: 0}
        for rep in range(2):
            e.launch()
            e.sync()
            done = _flow_octree_done(orbgpu_mod, e, 2)
            assert set(done) == {0, 1} and all(done[f] > before[f] for f in done), \
                (case.name, "launch", rep, "the dataflow launch's octree tasks did not run", before, done)
            before = done
            for f, (c, (*exp, items)) in enumerate(zip(pair, exps)):
                kps, desc = e.results(f)
                _check(f"dataflow launch of 2, frame {f}, launch {rep}", c, variant, items, exp,
                       e.debug_candidates(0, f), e.debug_level_keypoints(0, f), kps, desc)
    finally:
        e.close()


def test_one_level_of_3000_features_is_refused(orbgpu_mod):
    """2,488 features is the most one level holds (2,496 nodes of 64 bytes in a CU's LDS); past it the call is refused
    with ORB_ERR_GEOMETRY, as before."""
    img = oc.frames()["big"].image()
    with pytest.raises(orbgpu_mod.OrbError) as ei:
        orbgpu_mod.ORBextractor(3000, 1.2, 1, oc.INI_TH, oc.MIN_TH)(img)
    assert ei.value.status == -4   # ORB_ERR_GEOMETRY
    with pytest.raises(orbgpu_mod.OrbError) as ei:
        orbgpu_mod.ORBextractor(2489, 1.2, 1, oc.INI_TH, oc.MIN_TH)(img)
    assert ei.value.status == -4
