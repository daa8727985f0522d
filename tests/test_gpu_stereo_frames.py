"""The stereo path from raw bytes to resident frames: raw synthetic pairs go through orb_remap_device (two maps),
orb_extract_batch_device and orb_frames_create_from_batch_stereo; mvuRight / mvDepth equal orb_stereo_batch_device's,
every handle equals orb_frame_create_from_extract called by hand, and the C++ mirror (tests/cpp_rectify) returns the
same bytes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import remap_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_rectify")
W, H = 160, 120
MB, MBF = f32(0.1), f32(0.1 * 90.0)
SENT = f32(-777.0)
IDENTITY = (90.0, 90.0, 80.0, 60.0, (0.0, 0.0, 0.0, 0.0))        # k[0] == 0: what rectified images give
MILD = (90.0, 89.5, 80.5, 59.25, (-0.02, 0.003, -0.0005, 0.0001))
NPAIRS = 3
LEVELS = 4        # a 160 x 120 image holds four pyramid levels of the extractor (a level needs 62 pixels a side)


@pytest.fixture(scope="module")
def L(orbgpu_mod):
    from orbgpu import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def m(orbgpu_mod):
    return orbgpu_mod.ORBmatcher(0.8, True)


class Dev:
    def __init__(self, L, h, a):
        a = np.ascontiguousarray(a)
        self.L, self.h, self.n = L, h, max(a.nbytes, 4)
        self.p = L.orb_device_alloc(h, self.n)
        assert self.p
        if a.nbytes:
            assert L.orb_memcpy_h2d(h, self.p, a.ctypes.data, a.nbytes) == 0

    def get(self, dtype):
        out = np.zeros(self.n // np.dtype(dtype).itemsize, dtype)
        assert self.L.orb_memcpy_d2h(self.h, out.ctypes.data, self.p, out.nbytes) == 0
        return out

    def close(self):
        self.L.orb_device_free(self.h, self.p)


@pytest.fixture(scope="module")
def chain(orbgpu_mod, L):
    """Two raw pairs and a third whose left image is flat, rectified on the device with a left and a right map and
    extracted as one batch of six frames; beside it, the same batch's orb_stereo_batch_device outputs."""
    pairs = [ref.raw_pair(orbgpu_mod, W, H, 5 + p) for p in range(2)]
    (_, mxL, myL), (_, mxR, myR) = pairs[0]
    raw = [img for pr in pairs for img, _, _ in pr] + [np.full((H, W), 90, np.uint8), pairs[0][1][0]]
    ext = orbgpu_mod.BatchExtractor(500, W, H, 2 * NPAIRS, nlevels=LEVELS)
    RL, RR = orbgpu_mod.Rectifier(ext, mxL, myL), orbgpu_mod.Rectifier(ext, mxR, myR)
    ext.upload_raw(np.stack(raw), [RL, RR])
    ext.launch()
    ext.sync()
    # the frames the extraction saw are the host definition's
    got = np.zeros((2 * NPAIRS, H, W), np.uint8)
    assert L.orb_memcpy_d2h(ext.h, got.ctypes.data, ext.d_frames, got.nbytes) == 0
    for f in range(2 * NPAIRS):
        assert np.array_equal(got[f], orbgpu_mod.remap_host(raw[f], *((mxL, myL) if f % 2 == 0 else (mxR, myR)))), f
    host = [tuple(a.copy() for a in ext.results(f)) for f in range(2 * NPAIRS)]
    assert all(len(host[f][0]) > 50 for f in (0, 1, 2, 3, 5)) and len(host[4][0]) == 0
    cap = ext.kp_cap
    bufs = [Dev(L, ext.h, np.full(NPAIRS * cap, SENT, f32)), Dev(L, ext.h, np.full(NPAIRS * cap, SENT, f32)),
            Dev(L, ext.h, np.full(NPAIRS, -5, np.int32))]
    ext.stereo(NPAIRS, MB, MBF, bufs[0].p, bufs[1].p, bufs[2].p)
    ext.sync()
    want = (bufs[0].get(f32), bufs[1].get(f32), bufs[2].get(np.int32))
    assert want[2][0] > 5 and want[2][1] > 5 and want[2][2] == 0
    yield ext, host, want
    for b in bufs:
        b.close()
    RL.close()
    RR.close()
    ext.close()


def _queries(orbgpu, k_un, desc, uright, seed):
    """The frame's own features as projections, ur around their uright: the stereo gate passes some and drops others."""
    rng = np.random.default_rng(seed)
    sel = rng.permutation(len(k_un))[:60]
    q = orbgpu.proj_queries(k_un["x"][sel] + f32(0.5), k_un["y"][sel] - f32(0.5), np.full(len(sel), 8.0, f32),
                            k_un["octave"][sel], ur=uright[sel] + rng.uniform(-4, 4, len(sel)).astype(f32),
                            level_above=1, angle=k_un["angle"][sel])
    q["ur_tol"] = 2.0
    return q, desc[sel]


@pytest.mark.parametrize("cam", [IDENTITY, MILD], ids=["identity", "mild"])
def test_stereo_batch_constructor(orbgpu_mod, L, m, chain, cam):
    ext, host, (want_ur, want_d, want_n) = chain
    cap = ext.kp_cap
    dist = orbgpu_mod.distortion(*cam)
    bounds = tuple(orbgpu_mod.image_bounds(dist, W, H))
    bufs = [Dev(L, ext.h, np.full(NPAIRS * cap, SENT, f32)), Dev(L, ext.h, np.full(NPAIRS * cap, SENT, f32))]
    d_ur, d_dep = bufs
    frames, again = [], []
    try:
        frames = orbgpu_mod.Frame.from_batch_stereo(ext, dist, NPAIRS, MB, MBF, ext.d_desc, ext.d_kps, ext.d_counts, cap,
                                                    bounds=bounds, d_uright=d_ur.p, d_depth=d_dep.p)
        got_ur, got_d = d_ur.get(f32), d_dep.get(f32)
        # mvuRight / mvDepth: orb_stereo_batch_device's bytes, slots past each left count untouched
        assert got_ur.tobytes() == want_ur.tobytes() and got_d.tobytes() == want_d.tobytes()
        assert [len(F) for F in frames] == [len(host[0][0]), len(host[2][0]), 0]
        gated = 0
        for p, F in enumerate(frames):
            k, desc = host[2 * p]
            n, d_desc, d_kps = ext.frame_slots(2 * p)
            # by hand: the left slot's raw keypoints and descriptors with the pair's uright
            G = orbgpu_mod.Frame.from_extraction(ext, dist, n, d_desc, d_kps, bounds=bounds, d_uright=d_ur.p + 4 * p * cap)
            try:
                (off_f, idx_f), (off_g, idx_g) = F.grid(), G.grid()
                assert np.array_equal(off_f, off_g) and np.array_equal(idx_f, idx_g)
                if n:
                    un = orbgpu_mod.undistort_points_host(dist, np.stack([k["x"], k["y"]], 1))
                    k_un = k.copy()
                    k_un["x"], k_un["y"] = un[:, 0], un[:, 1]
                    ur = got_ur[p * cap:p * cap + n]
                    assert (ur > 0).sum() == want_n[p]
                    q, qd = _queries(orbgpu_mod, k_un, desc, ur, 7 + p)
                    a = m.search_by_projection(orbgpu_mod.PROJ_BEST, q, qd, frame=F, use_uright=True)
                    b = m.search_by_projection(orbgpu_mod.PROJ_BEST, q, qd, frame=G, use_uright=True)
                    c = m.search_by_projection(orbgpu_mod.PROJ_BEST, q, qd, frame=F, use_uright=False)
                    assert a[0] == b[0] > 0 and np.array_equal(a[1], b[1])
                    gated += int(not np.array_equal(a[1], c[1]))   # the gate changed the result: uright was read
            finally:
                G.close()
        assert gated > 0
        assert ext.results(0)[0].tobytes() == host[0][0].tobytes()   # the raw keypoints are not modified
        # without output arrays the handles are the same
        again = orbgpu_mod.Frame.from_batch_stereo(ext, dist, NPAIRS, MB, MBF, ext.d_desc, ext.d_kps, ext.d_counts, cap,
                                                   bounds=bounds)
        for F, G in zip(frames, again):
            assert len(F) == len(G) and all(np.array_equal(x, y) for x, y in zip(F.grid(), G.grid()))
        # fewer pairs than the batch holds is fine
        one = orbgpu_mod.Frame.from_batch_stereo(ext, dist, 1, MB, MBF, ext.d_desc, ext.d_kps, ext.d_counts, cap,
                                                 bounds=bounds)
        again += one
        assert all(np.array_equal(x, y) for x, y in zip(one[0].grid(), frames[0].grid()))
    finally:
        for F in frames + again:
            F.close()
        for b in bufs:
            b.close()


def test_stereo_constructor_refusals(orbgpu_mod, L, chain):
    """What needs a context to refuse: more pairs than the last batch holds, another kp_cap; and a count above kp_cap
    (ORB_ERR_CAPACITY), of a left and of a right slot, with out untouched."""
    ext, host, _ = chain
    cap = ext.kp_cap
    dist = orbgpu_mod.distortion(*IDENTITY)
    out = (ctypes.c_void_p * (NPAIRS + 1))(*([7] * (NPAIRS + 1)))

    def ctor(npairs=NPAIRS, kp_cap=cap, counts=ext.d_counts):
        return L.orb_frames_create_from_batch_stereo(ext.h, ctypes.byref(dist), npairs, float(MB), float(MBF), ext.d_desc,
                                                     ext.d_kps, counts, kp_cap, 0.0, 0.0, 0.4, 0.4, None, None, out)

    assert ctor(npairs=NPAIRS + 1) == -1 and b"fewer than" in L.orb_last_error()
    assert ctor(kp_cap=cap - 1) == -1 and b"kp_cap" in L.orb_last_error()
    assert all(v == 7 for v in out)
    counts = ext.counts()
    for slot in (2, 3):
        bad = counts.copy()
        bad[slot] = cap + 1
        d_bad = Dev(L, ext.h, bad)
        try:
            assert ctor(counts=d_bad.p) == -3, slot            # ORB_ERR_CAPACITY
            assert all(v == 7 for v in out)
        finally:
            d_bad.close()
    # and the context still works
    assert ctor() == 0 and all(v != 7 for v in out[:NPAIRS]) and out[NPAIRS] == 7
    for v in out[:NPAIRS]:
        L.orb_frame_destroy(v)


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_rectify_mirror")


def test_cpp_mirror(orbgpu_mod, mirror_bin, tmp_path):
    """The C++ Rectifier: its remap of both eyes, and operator() on the raw pair with ComputeStereoMatches behind it,
    against the Python mirror of the same C-ABI calls."""
    (rawL, mxL, myL), (rawR, mxR, myR) = ref.raw_pair(orbgpu_mod, W, H, 5)
    src, dst = tmp_path / "case.bin", tmp_path / "results.bin"
    with open(src, "wb") as fh:
        fh.write(np.array([W, H], np.int32).tobytes())
        fh.write(np.array([MB, MBF], f32).tobytes())
        for a in (mxL, myL, mxR, myR, rawL, rawR):
            fh.write(np.ascontiguousarray(a).tobytes())
    p = subprocess.run([mirror_bin, str(src), str(dst), str(LEVELS)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    buf = dst.read_bytes()
    el, er = orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7), orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7)
    RL, RR = orbgpu_mod.Rectifier(el, mxL, myL), orbgpu_mod.Rectifier(er, mxR, myR)
    try:
        pos = 0
        for R, raw in ((RL, rawL), (RR, rawR)):
            assert buf[pos:pos + W * H] == R.remap(raw).tobytes()
            pos += W * H
        kl, dl = el(rawL, rectify=RL)
        kr, dr = er(rawR, rectify=RR)
        u, d, n = orbgpu_mod.compute_stereo_matches(el, er, kl, dl, kr, dr, MB, MBF)
        for k, desc in ((kl, dl), (kr, dr)):
            cnt = int(np.frombuffer(buf, np.int32, 1, pos)[0])
            assert cnt == len(k) > 50
            assert buf[pos + 4:pos + 4 + 28 * cnt] == k.tobytes()
            assert buf[pos + 4 + 28 * cnt:pos + 4 + 60 * cnt] == desc.tobytes()
            pos += 4 + 60 * cnt
        nm = int(np.frombuffer(buf, np.int32, 1, pos)[0])
        assert nm == n > 5
        assert buf[pos + 4:pos + 4 + 4 * len(kl)] == u.tobytes()
        assert buf[pos + 4 + 4 * len(kl):pos + 4 + 8 * len(kl)] == d.tobytes()
        assert pos + 4 + 8 * len(kl) == len(buf)
    finally:
        RL.close()
        RR.close()
        el.close()
        er.close()
