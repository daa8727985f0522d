"""BoW on a resident frame (orb_frame_compute_bow: k_vocab_transform over the handles' descriptors, k_frame_featvec):
Frame.bow() equals ORBVocabulary.transform on the same descriptors, BowVector and FeatureVector, exactly
(tests/test_gpu_vocab.py pins transform to the oracle).  Sizes on both sides of a wavefront, of the workgroup's tile of
1,024 keys, none and one; one node holding everything; everything stopped; a batch with an empty frame inside."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BOUNDS = (0.0, 640.0, 0.0, 480.0)


@pytest.fixture(scope="module")
def vocs(orbgpu_mod, tmp_path_factory):
    """(vocabulary, levelsup) pairs: k = 10, L = 3; the second has stopped words."""
    from orbgpu.synth import write_synth_vocab
    d = tmp_path_factory.mktemp("voc")
    out = []
    for seed, stop, levelsup in ((5, 0.0, 1), (6, 0.3, 2)):
        path = str(d / f"voc_{seed}.bin")
        write_synth_vocab(path, 10, 3, seed=seed, stop_frac=stop)
        v = orbgpu_mod.ORBVocabulary()
        v.loadFromBinaryFile(path)
        out.append((v, levelsup))
    yield out
    for v, _ in out:
        v.close()


def _frame(orbgpu, ctx, desc):
    k = np.zeros(len(desc), orbgpu.KP_DTYPE)
    k["x"], k["y"] = 100.0, 100.0
    return orbgpu.Frame(ctx, desc, k, bounds=BOUNDS)


def _check(orbgpu, v, levelsup, descs):
    """compute_bow over one handle per descriptor set, in one call; every handle against transform()."""
    frames = [_frame(orbgpu, v, d) for d in descs]
    try:
        assert not any(F.has_bow for F in frames)
        orbgpu.compute_bow(v, frames, levelsup)
        for F, d in zip(frames, descs):
            assert F.has_bow
            want_bow, want_fv = v.transform(d, levelsup)
            bow, fv = F.bow(v)
            assert list(fv.keys()) == list(want_fv.keys()) and fv == want_fv, len(d)
            assert list(bow.keys()) == list(want_bow.keys()) and bow == want_bow, len(d)   # doubles, bit for bit
    finally:
        for F in frames:
            F.close()


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 257, 1100))
def test_featvec_sizes(orbgpu_mod, vocs, which, n):
    v, levelsup = vocs[which]
    desc = np.random.default_rng(100 + n).integers(0, 256, (n, 32), dtype=np.uint8)
    if which == 1 and n >= 63:
        _, wt, _ = v.transform_each(desc, levelsup)
        assert (wt <= 0).any() and (wt > 0).any()   # stopped words occur
    _check(orbgpu_mod, v, levelsup, [desc])


@pytest.mark.parametrize("n", (1, 65, 300, 1100))
def test_all_features_in_one_node(orbgpu_mod, vocs, n):
    v, levelsup = vocs[0]
    one = np.random.default_rng(9).integers(0, 256, (1, 32), dtype=np.uint8)
    desc = np.repeat(one, n, axis=0)
    _, fv = v.transform(desc, levelsup)
    assert len(fv) == 1
    _check(orbgpu_mod, v, levelsup, [desc])


def test_every_feature_stopped(orbgpu_mod, vocs):
    v, levelsup = vocs[1]
    rng = np.random.default_rng(12)
    pool = rng.integers(0, 256, (4000, 32), dtype=np.uint8)
    _, wt, _ = v.transform_each(pool, levelsup)
    stopped = pool[wt <= 0]
    assert 70 <= len(stopped)
    desc = stopped[:70]
    bow, fv = v.transform(desc, levelsup)
    assert bow == {} and fv == {}
    _check(orbgpu_mod, v, levelsup, [desc])


def test_batch_of_four_with_an_empty_frame(orbgpu_mod, vocs):
    v, levelsup = vocs[1]
    rng = np.random.default_rng(13)
    descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (300, 0, 65, 1030)]
    _check(orbgpu_mod, v, levelsup, descs)


def test_attaching_again_replaces(orbgpu_mod, vocs):
    """compute_bow twice with different levelsup, then set_featvec: each attach replaces the last."""
    v, _ = vocs[0]
    desc = np.random.default_rng(14).integers(0, 256, (200, 32), dtype=np.uint8)
    F = _frame(orbgpu_mod, v, desc)
    try:
        for levelsup in (1, 2, 1):
            F.compute_bow(v, levelsup)
            assert F.bow(v) == v.transform(desc, levelsup)
        given = {7: [3, 1], 9: [0]}
        F.set_featvec(given, v)
        assert F.has_bow and F.bow() == ({}, given)
    finally:
        F.close()
