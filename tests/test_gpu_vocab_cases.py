"""GPU parity of the vocabulary loader and k_vocab_transform / orb_vocab_bow (csrc/vocab.hip) with tests/vocab_ref.py
on the hand-written vocabulary of tests/vocab_cases.py: word ids, weights and node ids per feature for 1, 255, 256 and
257 features at every levelsup, the assembled BowVector and FeatureVector, and every scoring / weighting pair.  Where
the reference leaves the node id uninitialised (a leaf above nid_level) the product must return 0.
tests/test_vocab_cases.py checks on the CPU that the file and the features realise what they are named for."""
import numpy as np
import pytest

import vocab_cases as vc
import vocab_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loaded(orbgpu_mod, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("voc") / "planted.bin")
    vc.write(path)
    gv = orbgpu_mod.ORBVocabulary()
    gv.loadFromBinaryFile(path)
    yield gv, ref.Vocabulary(path)
    gv.close()


def test_loaded_shape(loaded):
    gv, v = loaded
    assert (gv.k, gv.L, gv.scoring, gv.weighting, gv.nnodes, gv.nwords) == (v.k, v.L, 0, 0, len(v.nodes), len(v.words))


@pytest.mark.parametrize("item", sorted(vc.LEVELSUP))
@pytest.mark.parametrize("n", vc.COUNTS)
def test_transform_matches_reference(loaded, n, item):
    gv, v = loaded
    levelsup = vc.LEVELSUP[item]
    feats, who = vc.features(n, seed=n)
    want = [v.transform_one(f, levelsup) for f in feats]
    w, wt, nd = gv.transform_each(feats, levelsup)
    want_nd = [0 if r[2] is None else r[2] for r in want]         # uninitialised upstream: the documented 0
    bad = [(i, who[i], int(w[i]), float(wt[i]), int(nd[i]), want[i][:3]) for i in range(n)
           if (int(w[i]), float(wt[i]), int(nd[i])) != (want[i][0], want[i][1], want_nd[i])]
    assert not bad, (n, item, bad[:8])
    bow, fv = v.transform(feats, levelsup)
    gbow, gfv = gv.transform(feats, levelsup)
    assert gbow == bow and list(gbow) == list(bow), (n, item)
    if None in fv:
        fv = dict(sorted(({0 if k is None else k: x for k, x in fv.items()}).items())) if 0 not in fv else None
    if fv is not None:
        assert gfv == fv and list(gfv) == list(fv), (n, item)


@pytest.mark.parametrize("scoring,weighting", vc.PAIRS)
def test_scoring_weighting_pairs(orbgpu_mod, tmp_path, scoring, weighting):
    path = str(tmp_path / "v.bin")
    vc.write(path, scoring, weighting)
    v = ref.Vocabulary(path)
    gv = orbgpu_mod.ORBVocabulary()
    gv.loadFromBinaryFile(path)
    try:
        for names in (vc.ALL_STOPPED, vc.SHARED):
            feats, _ = vc.features(len(names) * 2, seed=7, names=names)
            bow, fv = v.transform(feats, 2)
            gbow, gfv = gv.transform(feats, 2)
            assert gbow == bow and gfv == fv, (scoring, weighting, names, gbow, bow)
    finally:
        gv.close()
