"""GPU: two buffers of a context that grow past their floor between calls, each result compared with a fresh context
given the large input directly (and with the oracle / numpy): the matcher's pinned mirror (1 MiB floor, Stage::alloc)
and the device pair list with its pinned slots of orb_hamming_top2_frames_device (4096-byte floor).  The other
reallocation paths are crossed by tests that already exist: the keyframe pool by kfdb_cases.mutation_script, the
birdview geometry, mask pyramids and keypoint buffers by test_gpu_bird_batch.test_reuse_one_object."""
import ctypes

import numpy as np
import pytest

import top2_cases as tc

pytestmark = pytest.mark.gpu


def test_matcher_mirror_grows_past_its_floor(orbgpu_mod, oracle_mod, tmp_path):
    """orb_vocab_transform stages 44 bytes per descriptor in the pinned mirror: 40 descriptors stay under the 1 MiB
    floor, 26,000 need 1.1 MB.  Small, large, small again on one context; the large call also on a fresh one."""
    from orbgpu.synth import write_synth_vocab
    path = str(tmp_path / "voc.bin")
    write_synth_vocab(path, 6, 3, seed=11)
    desc = np.random.default_rng(23).integers(0, 256, (26000, 32), dtype=np.uint8)
    assert 44 * 40 + 8192 < (1 << 20) < 44 * len(desc)
    ow, owt, ond = oracle_mod.OracleVocabulary(path).transform_each(desc, 1)
    a, b = orbgpu_mod.ORBVocabulary(), orbgpu_mod.ORBVocabulary()
    try:
        a.loadFromBinaryFile(path)
        b.loadFromBinaryFile(path)
        fresh = b.transform_each(desc, 1)
        for n in (40, len(desc), 40, len(desc)):
            got = a.transform_each(desc[:n], 1)
            for g, f in zip(got, fresh):
                assert np.array_equal(g, f[:n]), n
        assert np.array_equal(fresh[0], ow) and np.array_equal(fresh[2], ond)
        assert np.array_equal(fresh[1].astype(np.float64), owt)
    finally:
        a.close()
        b.close()


def _top2_frames(bx, L, d_desc, d_counts, cap, qf, tf, d_out):
    from orbgpu import check
    qf, tf = np.ascontiguousarray(qf, np.int32), np.ascontiguousarray(tf, np.int32)
    check(L.orb_hamming_top2_frames_device(bx.h, d_desc, d_counts, cap, len(qf), ctypes.c_void_p(qf.ctypes.data),
                                           ctypes.c_void_p(tf.ctypes.data), *d_out), "orb_hamming_top2_frames_device")
    bx.sync()
    res = []
    for d in d_out:
        r = np.zeros(len(qf) * cap, np.int32)
        check(L.orb_memcpy_d2h(bx.h, r.ctypes.data, d, r.nbytes), "d2h")
        res.append(r.reshape(len(qf), cap))
    return res


def test_top2_pair_list_grows_past_its_floor(orbgpu_mod):
    """A list of 2 pairs (the 4096-byte floor), another of 600 (4800 bytes: the device list and a pinned slot are
    reallocated), then the first again, on one context; the 600 also as a fresh context's first call."""
    from orbgpu import _lib, check
    L = _lib.lib()
    F, cap = 8, 96
    rng = np.random.default_rng(41)
    desc = rng.integers(0, 256, (F, cap, 32), dtype=np.uint8)
    counts = np.array([96, 50, 64, 5, 77, 96, 33, 80], np.int32)
    small = ([0, 2], [1, 3])
    big = ([p % F for p in range(600)], [(3 * p + 1) % F for p in range(600)])
    assert len(small[0]) * 8 < 4096 < len(big[0]) * 8
    want = {(q, t): tc.top2_numpy(desc[q, :counts[q]], desc[t, :counts[t]]) for q in range(F) for t in range(F)}

    def session(lists):
        bx = orbgpu_mod.BatchExtractor(500, 320, 240, 1)   # (used for its handle, allocations and stream only)
        try:
            d_desc, d_counts = bx._alloc(desc.nbytes), bx._alloc(counts.nbytes)
            d_out = [bx._alloc(600 * cap * 4) for _ in range(3)]
            check(L.orb_memcpy_h2d(bx.h, d_desc, desc.ctypes.data, desc.nbytes), "h2d")
            check(L.orb_memcpy_h2d(bx.h, d_counts, counts.ctypes.data, counts.nbytes), "h2d")
            out = [_top2_frames(bx, L, d_desc, d_counts, cap, qf, tf, d_out) for qf, tf in lists]
            for d in [d_desc, d_counts] + d_out:
                L.orb_device_free(bx.h, d)
            return out
        finally:
            bx.close()

    lists = [small, big, small, big]
    got = session(lists)
    fresh = session([big])[0]
    for (qf, tf), res in zip(lists, got):
        for p, (q, t) in enumerate(zip(qf, tf)):
            n = counts[q]
            for r, w in zip(res, want[(q, t)]):
                assert np.array_equal(r[p, :n], w), (len(qf), p, q, t)
    for r, f in zip(got[1], fresh):
        for p, q in enumerate(big[0]):
            assert np.array_equal(r[p, :counts[q]], f[p, :counts[q]]), p
