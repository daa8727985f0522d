"""GPU: k_undistort_fisheye against the host twin (orb_undistort_points_host, pinned to the restatement by
tests/test_undistort_ref.py), byte for byte over all 28 bytes of a keypoint; the guard band; and the creators that make
resident frames from an extraction's raw output (orb_frame_create_from_extract, orb_frames_create_from_batch)."""
import ctypes

import numpy as np
import pytest

import projection_cases as pc
import undistort_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
IDENTITY = (350.0, 351.0, 160.0, 120.0, (0.0, 1.0, 1.0, 1.0))
CALS = dict(ref.CALIBRATIONS, identity=IDENTITY, branch=ref.BRANCH)
W, H = 320, 240
SMALL = (210.0, 209.0, 161.5, 118.25, (-0.02, 0.003, -0.0005, 0.0001))   # a mild camera of a 320 x 240 image
SENT = 0xA5


@pytest.fixture(scope="module")
def m(orbgpu_mod):
    return orbgpu_mod.ORBmatcher(0.8, True)


def _L():
    from orbgpu import _lib
    return _lib.lib()


class Dev:
    """Device buffers of one context, freed together."""

    def __init__(self, ctx_h):
        self.h, self.ptrs = ctx_h, []

    def alloc(self, nbytes, fill=None):
        p = _L().orb_device_alloc(self.h, max(int(nbytes), 4))
        assert p
        self.ptrs.append(p)
        if fill is not None:
            assert _L().orb_memset_device(self.h, p, fill, max(int(nbytes), 4)) == 0
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            assert _L().orb_memcpy_h2d(self.h, p, ctypes.c_void_p(a.ctypes.data), a.nbytes) == 0
        return p

    def down(self, p, dtype, count):
        out = np.zeros(count, dtype)
        if out.nbytes:
            assert _L().orb_memcpy_d2h(self.h, ctypes.c_void_p(out.ctypes.data), p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.ptrs:
            _L().orb_device_free(self.h, p)
        self.ptrs = []


@pytest.fixture()
def dev(m):
    d = Dev(m._ctx.h)
    yield d
    d.close()


def _keypoints(orbgpu, xy, seed):
    """Keypoints at xy whose other 24 bytes are random bits (they must come back unchanged)."""
    rng = np.random.default_rng(seed)
    k = np.zeros(len(xy), orbgpu.KP_DTYPE)
    k.view(np.uint8).reshape(len(xy), 28)[:] = rng.integers(0, 256, (len(xy), 28), dtype=np.uint8)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    return k


def _expected(orbgpu, cal, k):
    """k with x, y replaced by the host twin's."""
    un = orbgpu.undistort_points_host(orbgpu.distortion(*cal), np.stack([k["x"], k["y"]], 1))
    out = k.copy()
    out["x"], out["y"] = un[:, 0], un[:, 1]
    return out


def _points(cal, n, seed):
    return ref.seeded_points(cal, W, H, max(n, 16), seed)[:n]


def test_point_sets_reach_every_path():
    """What the sets below contain, by the restatement: the principal point, the pi/2 clip, both sides of
    theta_d > 1e-8 (the calibration whose principal point is the origin), and (the reference's calibration) a theta
    past the pole."""
    for name, cal in dict(ref.CALIBRATIONS, branch=ref.BRANCH).items():
        p = _points(cal, 63, 1)
        s = [ref.undistort_scale(cal, x, y) for x, y in p]
        assert s[0][:2] == (0.0, 0.0) and not s[0][3], name
        assert any((a * a + b * b) ** 0.5 > ref.HALF_PI for a, b, _, _ in s), name
        if name == "branch":
            assert s[1][0] > 0 and not s[1][3] and s[2][3] and s[3][3]
    assert any(sc < 0 for _, _, sc, _ in (ref.undistort_scale(ref.YAML, x, y) for x, y in _points(ref.YAML, 63, 1)))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", sorted(CALS))
def test_kernel_equals_host_twin(orbgpu_mod, m, name, n):
    cal = CALS[name]
    k = _keypoints(orbgpu_mod, _points(cal, n, 7 * n + 1), n)
    got, redone = orbgpu_mod.undistort_keypoints(m, orbgpu_mod.distortion(*cal), k)
    want = _expected(orbgpu_mod, cal, k)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
    assert 0 <= redone <= n
    if name == "identity":
        assert got.tobytes() == k.tobytes() and redone == 0


@pytest.mark.parametrize("in_place", [False, True], ids=["to_output", "in_place"])
@pytest.mark.parametrize("name", sorted(CALS))
def test_batch_of_three_frames(orbgpu_mod, m, dev, name, in_place):
    """Counts {0, 65, kp_cap}: every frame's records equal the host twin's, slots past a count keep their bytes."""
    cal, cap = CALS[name], 130
    counts = np.array([0, 65, cap], np.int32)
    k = _keypoints(orbgpu_mod, _points(cal, 3 * cap, 11), 5)
    d_in, d_counts = dev.up(k), dev.up(counts)
    d_out = d_in if in_place else dev.alloc(3 * cap * 28, fill=SENT)
    redone = ctypes.c_int(-1)
    st = _L().orb_undistort_keypoints_device(m._ctx.h, ctypes.byref(orbgpu_mod.distortion(*cal)), 3, d_in, d_counts, cap,
                                             d_out, ctypes.byref(redone))
    assert st == 0 and 0 <= redone.value <= counts.sum()
    got = dev.down(d_out, orbgpu_mod.KP_DTYPE, 3 * cap)
    want = k.copy() if in_place else np.frombuffer(bytes([SENT]) * (3 * cap * 28), orbgpu_mod.KP_DTYPE).copy()
    full = _expected(orbgpu_mod, cal, k)
    for f, c in enumerate(counts):
        want[f * cap:f * cap + c] = full[f * cap:f * cap + c]
    assert got.tobytes() == want.tobytes()
    if not in_place:
        assert dev.down(d_in, orbgpu_mod.KP_DTYPE, 3 * cap).tobytes() == k.tobytes()


def _guaranteed(orbgpu, cal, p):
    """The points of p whose results must differ across a guard band of 2^-20, by the reference arithmetic alone: the
    band moves a coordinate by 2^-19 |out - c| between its ends, and two doubles further apart than one float ulp
    (at most 2^-23 |out|) round to different floats.  So |out - c| > |out| / 16 in either coordinate suffices; the test
    asks for |out| / 8, and for the iteration branch."""
    fx, fy, cx, cy, _ = ref.calib32(cal)
    un = orbgpu.undistort_points_host(orbgpu.distortion(*cal), p).astype(np.float64)
    it = np.array([ref.undistort_scale(cal, x, y)[3] for x, y in p])
    far = (np.abs(un[:, 0] - cx) > np.abs(un[:, 0]) / 8) | (np.abs(un[:, 1] - cy) > np.abs(un[:, 1]) / 8)
    return p[it & far & np.isfinite(un).all(1)]


@pytest.mark.parametrize("name", sorted(ref.CALIBRATIONS))
def test_guard_band(orbgpu_mod, m, name):
    cal = ref.CALIBRATIONS[name]
    p = _guaranteed(orbgpu_mod, cal, _points(cal, 600, 21))
    assert len(p) > 200
    k = _keypoints(orbgpu_mod, p, 9)
    d, want = orbgpu_mod.distortion(*cal), _expected(orbgpu_mod, cal, k)
    try:
        orbgpu_mod.undistort_guard(m, 2.0 ** -20)
        got, redone = orbgpu_mod.undistort_keypoints(m, d, k)
        print(f"{name}: g = 2^-20 redid {redone} of {len(k)}")
        assert got.tobytes() == want.tobytes()
        assert redone == len(k)
    finally:
        orbgpu_mod.undistort_guard(m, 0.0)
    got, redone = orbgpu_mod.undistort_keypoints(m, d, k)
    print(f"{name}: the default band redid {redone} of {len(k)}")
    assert got.tobytes() == want.tobytes() and 0 <= redone <= len(k)
    # the identity path and the scale = 1 branch are never redone, however wide the band
    try:
        orbgpu_mod.undistort_guard(m, 2.0 ** -20)
        near = np.array([(ref.calib32(cal)[2], ref.calib32(cal)[3])] * 5, f32)
        assert orbgpu_mod.undistort_keypoints(m, d, _keypoints(orbgpu_mod, near, 1))[1] == 0
        assert orbgpu_mod.undistort_keypoints(m, orbgpu_mod.distortion(*IDENTITY), k)[1] == 0
    finally:
        orbgpu_mod.undistort_guard(m, 0.0)


# ---------------------------------------------------------------- resident frames from an extraction

@pytest.fixture(scope="module")
def extraction(orbgpu_mod):
    """Three 320 x 240 frames extracted on the device, the last one flat (no keypoint)."""
    from orbgpu.synth import synth_frame
    ext = orbgpu_mod.BatchExtractor(300, W, H, 3)
    frames = np.stack([synth_frame(W, H, 3), synth_frame(W, H, 4), np.full((H, W), 90, np.uint8)])
    ext.upload(frames)
    ext.launch()
    ext.sync()
    host = [ext.results(f) for f in range(3)]
    assert len(host[0][0]) > 100 and len(host[1][0]) > 100 and len(host[2][0]) == 0
    yield ext, host
    ext.close()


def _search(orbgpu, m, F, k_un, desc, seed):
    """SearchByProjection's core over the frame with the (undistorted) features themselves as projections."""
    rng = np.random.default_rng(seed)
    shifted = k_un.copy()
    shifted["x"] -= pc.DX
    shifted["y"] -= pc.DY
    sel, u, v, qd = pc._projected(rng, shifted, desc, 1.0, min(20, len(k_un)))
    q = orbgpu.proj_queries(u, v, np.full(len(sel), 6.0, f32), k_un["octave"][sel], level_above=1, angle=k_un["angle"][sel])
    return m.search_by_projection(orbgpu.PROJ_BEST, q, qd, frame=F)


def _same_frame(orbgpu, m, F, G, k_un, desc):
    assert len(F) == len(G) == len(k_un)
    (off_f, idx_f), (off_g, idx_g) = F.grid(), G.grid()
    assert np.array_equal(off_f, off_g) and np.array_equal(idx_f, idx_g)
    if len(k_un):
        (nf, mf), (ng, mg) = _search(orbgpu, m, F, k_un, desc, 5), _search(orbgpu, m, G, k_un, desc, 5)
        assert nf == ng > 0 and np.array_equal(mf, mg)


@pytest.mark.parametrize("guard", [0.0, 2.0 ** -20], ids=["default_band", "wide_band"])
def test_frame_from_extract(orbgpu_mod, m, extraction, guard):
    """The handle equals orb_frame_create's over the host-twin-undistorted keypoints and orb_image_bounds' bounds; with
    the wide band nearly every point is patched, which the grid must already see."""
    ext, host = extraction
    d = orbgpu_mod.distortion(*SMALL)
    bounds = orbgpu_mod.image_bounds(d, W, H)
    assert bounds.tobytes() == ref.image_bounds(SMALL, W, H).tobytes()
    k, desc = host[0]
    k_un = _expected(orbgpu_mod, SMALL, k)
    n, d_desc, d_kps = ext.frame_slots(0)
    G = orbgpu_mod.Frame(m, desc, k_un, bounds=tuple(bounds))
    try:
        orbgpu_mod.undistort_guard(ext, guard)
        F = orbgpu_mod.Frame.from_extraction(ext, d, n, d_desc, d_kps, bounds=tuple(bounds))
    finally:
        orbgpu_mod.undistort_guard(ext, 0.0)
    try:
        _same_frame(orbgpu_mod, m, F, G, k_un, desc)
        assert ext.results(0)[0].tobytes() == k.tobytes()   # the extraction's raw keypoints are not modified
    finally:
        F.close()
        G.close()


def test_frame_from_extract_identity(orbgpu_mod, m, extraction):
    """k[0] == 0: the handle of orb_frame_create_device over the raw keypoints."""
    ext, host = extraction
    k, desc = host[1]
    n, d_desc, d_kps = ext.frame_slots(1)
    b = (0.0, float(W), 0.0, float(H))
    assert orbgpu_mod.image_bounds(orbgpu_mod.distortion(*IDENTITY), W, H).tolist() == list(b)
    F = orbgpu_mod.Frame.from_extraction(ext, orbgpu_mod.distortion(*IDENTITY), n, d_desc, d_kps, bounds=b)
    G = orbgpu_mod.Frame.from_device(ext, n, d_desc, d_kps, bounds=b)
    try:
        _same_frame(orbgpu_mod, m, F, G, k, desc)
    finally:
        F.close()
        G.close()


def test_empty_frame_from_extract(orbgpu_mod, m, extraction):
    ext, _ = extraction
    F = orbgpu_mod.Frame.from_extraction(ext, orbgpu_mod.distortion(*SMALL), 0, None, None, bounds=(0.0, 320.0, 0.0, 240.0))
    off, idx = F.grid()
    F.close()
    assert len(F) == 0 and not off.any() and len(idx) == 0


@pytest.mark.parametrize("guard", [0.0, 2.0 ** -20], ids=["default_band", "wide_band"])
def test_frames_from_batch(orbgpu_mod, m, extraction, guard):
    """Each handle of the batch call equals its single-call counterpart; the flat frame gives an empty handle."""
    ext, host = extraction
    d = orbgpu_mod.distortion(*SMALL)
    bounds = tuple(orbgpu_mod.image_bounds(d, W, H))
    try:
        orbgpu_mod.undistort_guard(ext, guard)
        batch = orbgpu_mod.Frame.from_batch(ext, d, 3, ext.d_desc, ext.d_kps, ext.d_counts, ext.kp_cap, bounds=bounds)
    finally:
        orbgpu_mod.undistort_guard(ext, 0.0)
    try:
        assert [len(F) for F in batch] == [len(host[0][0]), len(host[1][0]), 0]
        for f, F in enumerate(batch):
            k, desc = host[f]
            n, d_desc, d_kps = ext.frame_slots(f)
            G = orbgpu_mod.Frame.from_extraction(ext, d, n, d_desc, d_kps, bounds=bounds)
            try:
                _same_frame(orbgpu_mod, m, F, G, _expected(orbgpu_mod, SMALL, k), desc)
            finally:
                G.close()
    finally:
        for F in batch:
            F.close()


def _free_bytes():
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert _L().hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_failing_batch_leaves_out_untouched_and_leaks_nothing(orbgpu_mod, extraction):
    ext, host = extraction
    d = orbgpu_mod.distortion(*SMALL)
    vp = ctypes.c_void_p
    out = (vp * 3)(*([0x5A5A] * 3))
    n0, n1 = len(host[0][0]), len(host[1][0])

    def call(kp_cap, inv_w):
        return _L().orb_frames_create_from_batch(ext.h, ctypes.byref(d), 3, vp(ext.d_desc), vp(ext.d_kps),
                                                 vp(ext.d_counts), kp_cap, 0.0, 0.0, inv_w, 0.2, out)

    # a kp_cap that holds the first frame's count but not the second's: the first handle exists when the call fails
    order = (0, 1) if n0 < n1 else (1, 0)
    small = len(host[order[0]][0])
    assert small < len(host[order[1]][0]), "the two frames' counts differ"
    if order == (1, 0):
        small = min(n0, n1) - 1   # (the first frame is the larger one: it is refused itself)
    assert call(small, 0.2) == -3   # ORB_ERR_CAPACITY
    before = _free_bytes()
    for _ in range(256):
        assert call(small, 0.2) == -3
    after = _free_bytes()
    # a handle leaked per call would be 256 allocations of tens of KiB each (at least 13 KiB: the grid alone)
    assert before - after < 256 * 13 * 1024 // 2, (before, after)
    assert call(ext.kp_cap, 0.0) == -1 and call(ext.kp_cap, float("nan")) == -1   # a bad grid argument
    assert all(h == 0x5A5A for h in out)
    assert call(ext.kp_cap, 0.2) == 0 and all(h != 0x5A5A and h for h in out)   # and the same call with nothing wrong
    for h in out:
        _L().orb_frame_destroy(vp(h))
