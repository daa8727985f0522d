"""SearchForTriangulation between resident frames (orb_search_for_triangulation_frames, k_triangulation_frames) against
the host-pointer entry points on the same arrays, exactly: the planted cases of tests/triangulation_cases.py (every
Plant realised), the batch, the edges of the node search, flags that change between two calls on the same handles,
the capacity error, the argument checks that need a live handle, and, end to end, frames that were extracted and had
their BoW computed on the device."""
import ctypes

import numpy as np
import pytest

import triangulation_cases as tc
from triangulation_cases import _T, P, Q

pytestmark = pytest.mark.gpu
BOUNDS = (0.0, 640.0, 0.0, 480.0)


@pytest.fixture(scope="module")
def m(orbgpu_mod):
    return orbgpu_mod.ORBmatcher(0.6, True)


class Handles:
    """Both sides of a case as Frames with uright and the case's FeatureVectors attached."""

    def __init__(self, orbgpu, m, c):
        self.F1 = orbgpu.Frame(m, c.desc1, c.kps1, bounds=BOUNDS, uright=c.ur1)
        self.F2 = orbgpu.Frame(m, c.desc2, c.kps2, bounds=BOUNDS, uright=c.ur2)
        self.F1.set_featvec(c.fv1, m)
        self.F2.set_featvec(c.fv2, m)

    def close(self):
        self.F1.close()
        self.F2.close()


def _other(c, F2=None, mp2=None):
    d = dict(has_mp2=c.mp2 if mp2 is None else mp2, F12=tc.F12, ex=tc.EX, ey=tc.EY, scale_factors2=tc.SCALE2,
             level_sigma2_2=tc.SIGMA2)
    if F2 is None:
        d.update(desc2=c.desc2, kps2=c.kps2, uright2=c.ur2, featvec2=c.fv2)
    else:
        d.update(frame2=F2)
    return d


def _host(m, c, only_stereo, mp1=None, mp2=None):
    return m.SearchForTriangulation(c.desc1, c.kps1, c.mp1 if mp1 is None else mp1, c.ur1, c.fv1, c.desc2, c.kps2,
                                    c.mp2 if mp2 is None else mp2, c.ur2, c.fv2, tc.F12, tc.EX, tc.EY, tc.SCALE2,
                                    tc.SIGMA2, bOnlyStereo=only_stereo)


def _variants():
    for name in tc.CASES:
        yield name, "as_built", tc.cases()[name]
        yield name, "reversed", tc.reversed_lists(tc.cases()[name])


@pytest.mark.parametrize("check_ori", (True, False))
@pytest.mark.parametrize("only_stereo", (False, True))
def test_planted_cases(orbgpu_mod, only_stereo, check_ori):
    m = orbgpu_mod.ORBmatcher(0.6, check_ori)
    bad = []
    for name, order, c in _variants():
        H = Handles(orbgpu_mod, m, c)
        try:
            got, = m.SearchForTriangulationFrames(H.F1, c.mp1, [_other(c, H.F2)], bOnlyStereo=only_stereo)
        finally:
            H.close()
        want = _host(m, c, only_stereo)
        if check_ori:
            ref, _ = tc.expected(c, only_stereo)
            assert np.array_equal(want, ref)
        if not np.array_equal(got, want):
            bad.append((name, order, got.tolist(), want.tolist()))
        if order == "as_built" and not check_ori:   # (no rotation cull: the loop's own answers)
            pairs = {int(a): int(b) for a, b in got}
            for p in c.plants:
                exp = p.best_stereo if only_stereo else p.best
                if exp is not None and pairs.get(p.idx1, -1) != exp:
                    bad.append((name, p.item, p.idx1, pairs.get(p.idx1, -1), exp))
    assert not bad, bad


@pytest.mark.parametrize("only_stereo", (False, True))
def test_batch_of_all_cases_against_the_first_kf1(orbgpu_mod, m, only_stereo):
    first = tc.cases()[tc.CASES[0]]
    variants = [c for _, _, c in _variants()]
    hs = [Handles(orbgpu_mod, m, c) for c in variants]
    try:
        got = m.SearchForTriangulationFrames(hs[0].F1, first.mp1, [_other(c, H.F2) for c, H in zip(variants, hs)],
                                             bOnlyStereo=only_stereo)
    finally:
        for H in hs:
            H.close()
    want = m.SearchForTriangulationBatch(first.desc1, first.kps1, first.mp1, first.ur1, first.fv1,
                                         [_other(c) for c in variants], bOnlyStereo=only_stereo)
    assert len(got) == len(want) == len(variants)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert sum(len(w) for w in want) > (0 if only_stereo else 20)   # (few planted pairs are stereo on both sides)


def _node_search_case():
    """KF1 nodes 2, 5, 9, 12, 20; a match is planted wherever KF2 has the node too."""
    b = _T("node_search", 77)
    q = {}
    for node in (2, 5, 9, 12, 20):
        q[node] = b.q(node)
    outside = b.rand()   # a KF1 feature in no node of its own FeatureVector, its exact copy a KF2 candidate
    return b, q, outside


def _finish(b, q, outside, kf2_nodes, extra2=()):
    for node in kf2_nodes:
        b.c(node, q[node][1], 7)
    for node in extra2:   # KF2 nodes KF1 lacks
        b.feat(2, node, b.rand(), P)
    c = b.done()
    n1 = len(c.desc1)
    desc1 = np.concatenate([c.desc1, outside[None, :]])
    kps1 = np.concatenate([c.kps1, c.kps1[:1]])
    c = c._replace(desc1=desc1, kps1=kps1, mp1=np.concatenate([c.mp1, [0]]).astype(np.uint8),
                   ur1=np.concatenate([c.ur1, [-1.0]]).astype(np.float32))
    return c, n1


@pytest.mark.parametrize("kf2_nodes,extra2", [((2,), ()), ((20,), ()), ((9,), ()), ((2, 20), (1, 30)), ((5, 12), (3, 6, 40)),
                                              ((2, 5, 9, 12, 20), ()), ((), (1, 3, 30)), ((), ())],
                         ids=["first_only", "last_only", "only_node", "first_and_last", "inner", "all", "disjoint", "empty_kf2"])
def test_node_search_edges(orbgpu_mod, m, kf2_nodes, extra2):
    b, q, outside = _node_search_case()
    if kf2_nodes or extra2:
        b.feat(2, (kf2_nodes + extra2)[0], outside.copy(), P)   # the outside feature's copy is a candidate somewhere
    c, n_in = _finish(b, q, outside, kf2_nodes, extra2)
    if not (kf2_nodes or extra2):
        c = c._replace(desc2=np.zeros((3, 32), np.uint8), kps2=np.zeros(3, tc.KP_DTYPE), mp2=np.zeros(3, np.uint8),
                       ur2=np.full(3, -1.0, np.float32), fv2={})   # features, but an empty FeatureVector
    H = Handles(orbgpu_mod, m, c)
    try:
        got, = m.SearchForTriangulationFrames(H.F1, c.mp1, [_other(c, H.F2)])
    finally:
        H.close()
    want = _host(m, c, False)
    assert np.array_equal(got, want)
    assert sorted(got[:, 0].tolist()) == sorted(q[node][0] for node in kf2_nodes)
    assert n_in not in got[:, 0]


def test_flags_are_fresh_per_call(orbgpu_mod, m):
    c = tc.cases()["edges"]
    rng = np.random.default_rng(5)
    H = Handles(orbgpu_mod, m, c)
    try:
        seen = set()
        for k in range(3):
            mp1 = c.mp1 if k == 0 else (rng.random(len(c.mp1)) < 0.3).astype(np.uint8)
            mp2 = c.mp2 if k == 0 else (rng.random(len(c.mp2)) < 0.3).astype(np.uint8)
            got, = m.SearchForTriangulationFrames(H.F1, mp1, [_other(c, H.F2, mp2)])
            assert np.array_equal(got, _host(m, c, False, mp1, mp2))
            seen.add(got.tobytes())
        assert len(seen) == 3
    finally:
        H.close()


def test_capacity_one_short(orbgpu_mod, m):
    c = tc.cases()["edges"]
    want = _host(m, c, False)
    H = Handles(orbgpu_mod, m, c)
    try:
        with pytest.raises(orbgpu_mod.OrbError) as e:
            m.SearchForTriangulationFrames(H.F1, c.mp1, [_other(c, H.F2), _other(c, H.F2)], cap=len(want) - 1)
        assert e.value.status == -3
        assert [n.value for n in m.last_tri_counts] == [len(want), len(want)]
        got = m.SearchForTriangulationFrames(H.F1, c.mp1, [_other(c, H.F2)], cap=len(want))
        assert np.array_equal(got[0], want)
    finally:
        H.close()


def test_argument_checks_that_need_a_handle(orbgpu_mod, m):
    """ORB_ERR_ARG, nothing written: a handle without BoW, one without uright, a FeatureVector index >= n, a frame2
    octave the level tables do not cover."""
    from orbgpu import _lib
    L = _lib.lib()
    c = tc.cases()["rot_tied"]
    H = Handles(orbgpu_mod, m, c)
    bare = orbgpu_mod.Frame(m, c.desc2, c.kps2, bounds=BOUNDS, uright=c.ur2)
    no_ur = orbgpu_mod.Frame(m, c.desc2, c.kps2, bounds=BOUNDS)
    no_ur.set_featvec(c.fv2, m)
    try:
        def status(F1, F2, **kw):
            try:
                m.SearchForTriangulationFrames(F1, c.mp1, [dict(_other(c, F2), **kw)])
            except orbgpu_mod.OrbError as e:
                return e.status, L.orb_last_error().decode()
            return 0, ""

        fn = "orb_search_for_triangulation_frames: "
        assert status(H.F1, bare) == (-1, fn + "a frame carries no BoW")
        assert status(H.F1, no_ur) == (-1, fn + "a frame was created without uright")
        assert status(H.F1, H.F2, scale_factors2=tc.SCALE2[:1], level_sigma2_2=tc.SIGMA2[:1])[0] == 0   # octaves all 0
        edges = tc.cases()["edges"]
        E = Handles(orbgpu_mod, m, edges)
        try:
            assert status(H.F1, E.F2, has_mp2=edges.mp2, scale_factors2=tc.SCALE2[:1], level_sigma2_2=tc.SIGMA2[:1]) == \
                (-1, fn + "a frame2 octave outside [0, nlevels2)")
        finally:
            E.close()
        assert not bare.has_bow
        with pytest.raises(orbgpu_mod.OrbError) as e:
            bare.set_featvec({1: [0, len(c.desc2)]}, m)
        assert e.value.status == -1 and not bare.has_bow
        assert L.orb_last_error().decode() == "orb_frame_set_featvec: FeatureVector index outside the frame"
        with pytest.raises(orbgpu_mod.OrbError):
            bare.bow()
        kfs = [dict(frame=bare, mp=c.mp2)]
        with pytest.raises(orbgpu_mod.OrbError) as e:
            m.SearchByBoW_Frames_KF_F(kfs, H.F1)
        assert e.value.status == -1
    finally:
        H.close()
        bare.close()
        no_ur.close()


def test_end_to_end_from_a_device_batch(orbgpu_mod, m, tmp_path):
    """Two views extracted on the device become handles without leaving it (orb_frames_create_from_batch for the BoW
    search; orb_frame_create_device with a device uright for the triangulation, which needs mvuRight), get their BoW
    from orb_frame_compute_bow, and are searched; the host-pointer calls get the downloaded arrays and Frame.bow()."""
    from orbgpu import _lib
    from orbgpu.synth import synth_frame, write_synth_vocab
    L = _lib.lib()
    W, Hh = 320, 240
    path = str(tmp_path / "voc.bin")
    write_synth_vocab(path, 10, 3, seed=21)
    v = orbgpu_mod.ORBVocabulary()
    v.loadFromBinaryFile(path)
    ext = orbgpu_mod.BatchExtractor(300, W, Hh, 2)
    frames, urs, d_urs = [], [], []
    try:
        view = synth_frame(W, Hh, 3)
        ext.upload(np.stack([view, np.roll(view, 6, axis=1)]))   # the second view: the scene 6 px to the right
        ext.launch()
        ext.sync()
        host = [ext.results(f) for f in range(2)]
        assert min(len(k) for k, _ in host) > 100
        b = (0.0, float(W), 0.0, float(Hh))
        rng = np.random.default_rng(31)
        batch = orbgpu_mod.Frame.from_batch(ext, orbgpu_mod.distortion(100.0, 100.0, W / 2, Hh / 2, [0, 0, 0, 0]), 2,
                                            ext.d_desc, ext.d_kps, ext.d_counts, ext.kp_cap, bounds=b)
        frames += batch
        for f in range(2):
            n, d_desc, d_kps = ext.frame_slots(f)
            ur = np.where(rng.random(n) < 0.5, rng.uniform(0, W, n), -1.0).astype(np.float32)
            d_ur = L.orb_device_alloc(ext.h, max(n, 1) * 4)
            d_urs.append(d_ur)
            assert L.orb_memcpy_h2d(ext.h, d_ur, ur.ctypes.data, n * 4) == 0 and L.orb_sync(ext.h) == 0
            urs.append(ur)
            frames.append(orbgpu_mod.Frame.from_device(ext, n, d_desc, d_kps, bounds=b, d_uright=d_ur))
        orbgpu_mod.compute_bow(v, frames, 2)
        bows = [F.bow(v) for F in frames]
        for f in range(2):
            assert bows[f] == bows[2 + f] == v.transform(host[f][1], 2)
        (k1, desc1), (k2, desc2) = host
        fv1, fv2 = bows[0][1], bows[1][1]
        mp1 = (rng.random(len(k1)) < 0.4).astype(np.uint8)
        mp2 = (rng.random(len(k2)) < 0.4).astype(np.uint8)
        # SearchByBoW(KF = view 0, F = view 1)
        want = m.SearchByBoW_KF_F(desc1, k1["angle"], mp1, fv1, desc2, k2["angle"], fv2)
        (n_got, got), = m.SearchByBoW_Frames_KF_F([dict(frame=batch[0], mp=mp1)], batch[1])
        assert n_got == want[0] and np.array_equal(got, want[1]) and want[0] > 0
        # SearchForTriangulation(view 0, view 1): a fundamental matrix of a pure sideways motion (horizontal lines)
        F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
        lv = np.float32(1.2) ** np.arange(8, dtype=np.float32)
        other = dict(has_mp2=mp2, F12=F12, ex=-1000.0, ey=120.0, scale_factors2=lv, level_sigma2_2=lv * lv)
        for only_stereo in (False, True):
            want = m.SearchForTriangulation(desc1, k1, mp1, urs[0], fv1, desc2, k2, mp2, urs[1], fv2, F12, -1000.0, 120.0,
                                            lv, lv * lv, bOnlyStereo=only_stereo)
            got, = m.SearchForTriangulationFrames(frames[2], mp1, [dict(other, frame2=frames[3])], bOnlyStereo=only_stereo)
            assert np.array_equal(got, want)
        assert len(want) > 0
    finally:
        for F in frames:
            F.close()
        for d in d_urs:
            L.orb_device_free(ext.h, d)
        ext.close()
        v.close()
