"""GPU parity of the birdview ORB stream (csrc/bird.hip) on the planted cases of tests/bird_cases.py: every output
equals the oracle byte for byte (debug_candidates with the Harris bytes, detect, cornerSubPix, compute, extract), and
every plant holds in the GPU's own output: positions present or absent with their FAST scores, the counts of the tie
groups, the exact angles, the descriptors of tests/bird_ref.py where it states them, the unchanged and the reset
points bit-identical, the ideal corners within twice the measured distances.  tests/test_bird_cases.py checks on the
CPU that the cases realise the decisions they are named for.  A failure names the plant items involved."""
import numpy as np
import pytest

import bird_cases as bc

pytestmark = pytest.mark.gpu


def _bird(orbgpu_mod, case):
    return orbgpu_mod.BirdORB(case.nfeat, 1.2, case.nlevels, 31, 20)


def _report(case, what, equal, failures):
    """[] when the bytes equal the oracle's and every plant holds; otherwise the case, the stage, and the items."""
    items = sorted({it for it, _ in failures})
    if equal and not failures:
        return []
    return [(case.name, what, "bytes differ from the oracle" if not equal else "bytes equal",
             items or sorted({p.item for p in case.plants}), failures[:6])]


@pytest.mark.parametrize("name", [c.name for c in bc.by_kind("detect")])
def test_detect_case(orbgpu_mod, oracle_mod, name):
    case = bc.cases()[name]
    mask = oracle_mod.bird_footprint_mask(case.mask) if name == "footprint" else case.mask
    o = oracle_mod.OracleCvORB(case.nfeat, 1.2, case.nlevels)
    b = _bird(orbgpu_mod, case)
    try:
        ko, kg = o.detect(case.img, mask), b.detect(case.img, mask)
        co = [o.candidates(l) for l in range(case.nlevels)]
        cg = [b.debug_candidates(l) for l in range(case.nlevels)]
        same = all(len(g) == len(c) and all(np.array_equal(g[f], c[f]) for f in ("x", "y", "octave", "class_id")) and
                   g["response"].tobytes() == c["response"].tobytes() for g, c in zip(cg, co))
        assert not _report(case, "debug_candidates", same, bc.detect_failures(case, cg, kg))
        assert not _report(case, "detect", kg.tobytes() == ko.tobytes(), [])
        (ke, de), (kx, dx) = o.extract(case.img, case.mask), b.extract(case.img, case.mask)
        assert not _report(case, "extract", kx.tobytes() == ke.tobytes() and np.array_equal(dx, de),
                           bc.extract_failures(case, kx))
    finally:
        b.close()


@pytest.mark.parametrize("name", [c.name for c in bc.by_kind("subpix")])
def test_subpix_case(orbgpu_mod, oracle_mod, name):
    case = bc.cases()[name]
    b = orbgpu_mod.BirdORB(500, 1.2, 1, 31, 20)
    try:
        po, pg = oracle_mod.corner_subpix(case.img, case.pts), b.cornerSubPix(case.img, case.pts)
        bad = [i for i in range(len(pg)) if pg[i].tobytes() != po[i].tobytes()]
        items = sorted({p.item for p in case.plants if p.where in bad})
        fails = [(it, "differs from the oracle") for it in items] + bc.subpix_failures(case, pg)
        assert not _report(case, "cornerSubPix", not bad, fails)
    finally:
        b.close()


@pytest.mark.parametrize("name", [c.name for c in bc.by_kind("compute")])
def test_compute_case(orbgpu_mod, oracle_mod, name):
    case = bc.cases()[name]
    o = oracle_mod.OracleCvORB(case.nfeat, 1.2, case.nlevels)
    b = _bird(orbgpu_mod, case)
    try:
        (ko, do), (kg, dg) = o.compute(case.img, case.kps), b.compute(case.img, case.kps)
        fails = bc.compute_failures(case, kg, dg)
        if len(dg) == len(do):       # name the plants whose descriptors differ from the oracle's
            kept = bc.kept_inputs(case)
            rows = {kept[j] for j in np.flatnonzero((dg != do).any(1))} if len(kept) == len(dg) else set()
            fails += [(p.item, (p.where, "differs from the oracle")) for p in case.plants if p.what == "desc" and p.where in rows]
        assert not _report(case, "compute", kg.tobytes() == ko.tobytes() and np.array_equal(dg, do), fails)
    finally:
        b.close()


def test_batch_equals_single_frames(orbgpu_mod):
    """Every 192 x 160 planted frame (detect, cornerSubPix and compute images) with a mask of its own through one
    extract_batch call (more frames than batch_group, so several upload groups): frame by frame what extract returns."""
    cs, imgs, masks = bc.batch_frames()
    b = orbgpu_mod.BirdORB(500, 1.2, 1, 31, 20)
    try:
        assert len(imgs) > 2 * b.batch_group() > 0
        single = [b.extract(i, m) for i, m in zip(imgs, masks)]
        batch = b.extract_batch(imgs, list(masks))
        bad = [c.name for c, (ks, ds), (kb, db) in zip(cs, single, batch)
               if kb.tobytes() != ks.tobytes() or not np.array_equal(db, ds)]
        assert not bad, (bad, sorted({p.item for c in cs if c.name in bad for p in c.plants}))
        assert sum(len(k) for k, _ in single) > 500       # the textured frames give hundreds each
        fp = [c.name for c in cs].index("footprint")
        assert not bc.extract_failures(cs[fp], batch[fp][0])
    finally:
        b.close()
