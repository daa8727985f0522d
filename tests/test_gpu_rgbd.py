"""Frame::ComputeStereoFromRGBD on the GPU: k_rgbd_depth equals the CPU definition (orb_stereo_from_rgbd_host) and the
np.float32 restatement bit for bit on the planted case, the RGB-D batch constructor builds the frames orb_frame_create
builds over the host-undistorted keypoints with the host definition's uright, and the C++ and Python mirrors return
the C-ABI's bytes.  The C++ side runs as tests/cpp_rgbd/test_rgbd_mirror on a case written here."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import rgbd_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_rgbd")
W, H = 320, 240
SMALL = (210.0, 209.0, 161.5, 118.25, (-0.02, 0.003, -0.0005, 0.0001))   # a mild fisheye camera of a 320 x 240 image
TUM = f32(1.0) / f32(5000.0)
MBF = f32(40.0)
NCELL = 64 * 48 + 1
SENT = f32(-777.0)


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


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("factor", [TUM, f32(1.0)], ids=["tum", "one"])
def test_device_form_equals_the_host_definition(orbgpu_mod, L, m, kind, factor):
    counts = np.array([0, 1, 63, 64, 65, 200], np.int32)
    cap, nf = 200, len(counts)
    es = 2 if kind == "u16" else 4
    rs = ref.MAP_W * es + 3 * es                    # a row stride larger than the row
    fp = rs * ref.MAP_H + 5 * es
    maps = [ref.planted_map(kind, seed=5 + f) for f in range(nf)]
    mbuf = np.full(nf * fp, 0xEE, np.uint8)
    for f, mp in enumerate(maps):
        for y in range(ref.MAP_H):
            o = f * fp + y * rs
            mbuf[o:o + ref.MAP_W * es] = mp[y].view(np.uint8)
    k = np.zeros(nf * cap, orbgpu_mod.KP_DTYPE)
    ku = np.zeros(nf * cap, orbgpu_mod.KP_DTYPE)
    for f in range(nf):
        k[f * cap:(f + 1) * cap], ku[f * cap:(f + 1) * cap] = ref.planted_keypoints(cap, seed=20 + f,
                                                                                    with_outside=(f == nf - 1))
    want_ur = np.full(nf * cap, SENT, f32)
    want_d = np.full(nf * cap, SENT, f32)
    want_n = np.zeros(nf, np.int32)
    for f in range(nf):
        s = slice(f * cap, f * cap + counts[f])
        r_ur, r_d, r_n, outside = ref.stereo_from_rgbd(maps[f], factor, k[s], ku[s], MBF)
        assert outside.sum() == (2 if f == nf - 1 else 0)
        # the host definition on the keypoints it accepts; -1 / -1 for the two it refuses
        inside = np.flatnonzero(~outside)
        h_ur, h_d, h_n = orbgpu_mod.stereo_from_rgbd_host(maps[f], factor, k[s][inside], ku[s][inside], MBF)
        full_ur, full_d = np.full(counts[f], -1, f32), np.full(counts[f], -1, f32)
        full_ur[inside], full_d[inside] = h_ur, h_d
        assert full_ur.tobytes() == r_ur.tobytes() and full_d.tobytes() == r_d.tobytes() and h_n == r_n
        want_ur[s], want_d[s], want_n[f] = full_ur, full_d, h_n
    assert want_n[-1] > 50 and (want_d[5 * cap + 198:5 * cap + 200] == -1).all()
    h = m._ctx.h
    bufs = [Dev(L, h, a) for a in (mbuf, k, ku, counts, np.full(nf * cap, SENT, f32), np.full(nf * cap, SENT, f32),
                                   np.full(nf, -5, np.int32))]
    d_map, d_k, d_ku, d_cnt, d_ur, d_dep, d_nv = bufs
    try:
        dm = orbgpu_mod.depth_map(d_map.p, ref.DEPTH_U16 if kind == "u16" else ref.DEPTH_F32, ref.MAP_W, ref.MAP_H, rs, fp,
                                  factor)
        st = L.orb_stereo_from_rgbd_device(h, ctypes.byref(dm), float(MBF), nf, d_k.p, d_ku.p, d_cnt.p, cap, d_ur.p, d_dep.p,
                                           d_nv.p)
        assert st == 0 and L.orb_sync(h) == 0
        assert d_ur.get(f32).tobytes() == want_ur.tobytes()      # (slots past each count keep the sentinel)
        assert d_dep.get(f32).tobytes() == want_d.tobytes()
        assert np.array_equal(d_nv.get(np.int32), want_n)
    finally:
        for b in bufs:
            b.close()


@pytest.fixture(scope="module")
def extraction(orbgpu_mod):
    """Three 320 x 240 frames extracted on the device, the middle one flat (no keypoint)."""
    from orbgpu.synth import synth_frame
    ext = orbgpu_mod.BatchExtractor(300, W, H, 3)
    ext.upload(np.stack([synth_frame(W, H, 3), np.full((H, W), 90, np.uint8), synth_frame(W, H, 4)]))
    ext.launch()
    ext.sync()
    host = [tuple(a.copy() for a in ext.results(f)) for f in range(3)]
    assert len(host[0][0]) > 100 and len(host[1][0]) == 0 and len(host[2][0]) > 100
    yield ext, host
    ext.close()


def _depth_images(seed=31):
    rng = np.random.default_rng(seed)
    d = rng.integers(500, 65536, (3, H, W)).astype(np.uint16)
    d[rng.random((3, H, W)) < 0.25] = 0
    return d


def _expected_un(orbgpu, k):
    un = orbgpu.undistort_points_host(orbgpu.distortion(*SMALL), np.stack([k["x"], k["y"]], 1))
    out = k.copy()
    if len(k):
        out["x"], out["y"] = un[:, 0], un[:, 1]
    return out


def _gated_queries(orbgpu, k_un, desc, uright, seed):
    """The frame's own features as projections, ur around their uright: the stereo gate passes some and drops others."""
    rng = np.random.default_rng(seed)
    sel = rng.permutation(len(k_un))[:60]
    q = orbgpu.proj_queries(k_un["x"][sel] + f32(0.5), k_un["y"][sel] - f32(0.5), np.full(len(sel), 8.0, f32),
                            k_un["octave"][sel], ur=uright[sel] + rng.uniform(-4, 4, len(sel)).astype(f32),
                            level_above=1, angle=k_un["angle"][sel])
    q["ur_tol"] = 2.0
    return q, desc[sel]


def test_rgbd_batch_constructor(orbgpu_mod, L, m, extraction):
    ext, host = extraction
    cap = ext.kp_cap
    dist = orbgpu_mod.distortion(*SMALL)
    bounds = tuple(orbgpu_mod.image_bounds(dist, W, H))
    min_xy = (float(bounds[0]), float(bounds[2]))   # the staged form's grid origin (the handle keeps its own)
    depth = _depth_images()
    bufs = [Dev(L, ext.h, a) for a in (depth, np.full(3 * cap, SENT, f32), np.full(3 * cap, SENT, f32))]
    d_map, d_ur, d_dep = bufs
    frames = []
    try:
        dm = orbgpu_mod.depth_map(d_map.p, ref.DEPTH_U16, W, H, factor=TUM)
        frames = orbgpu_mod.Frame.from_batch_rgbd(ext, dist, dm, MBF, 3, ext.d_desc, ext.d_kps, ext.d_counts, cap,
                                                  bounds=bounds, d_uright=d_ur.p, d_depth=d_dep.p)
        got_ur, got_d = d_ur.get(f32), d_dep.get(f32)
        assert [len(F) for F in frames] == [len(host[0][0]), 0, len(host[2][0])]
        gated = 0
        for f, F in enumerate(frames):
            k, desc = host[f]
            k_un = _expected_un(orbgpu_mod, k)
            ur, dep, nv = orbgpu_mod.stereo_from_rgbd_host(depth[f], TUM, k, k_un, MBF)
            r_ur, r_d, r_n, outside = ref.stereo_from_rgbd(depth[f], TUM, k, k_un, MBF)
            assert not outside.any() and ur.tobytes() == r_ur.tobytes() and dep.tobytes() == r_d.tobytes() and nv == r_n
            s = slice(f * cap, f * cap + len(k))
            assert got_ur[s].tobytes() == ur.tobytes() and got_d[s].tobytes() == dep.tobytes()
            assert (got_ur[f * cap + len(k):(f + 1) * cap] == SENT).all()
            assert (got_d[f * cap + len(k):(f + 1) * cap] == SENT).all()
            G = orbgpu_mod.Frame(m, desc, k_un, bounds=bounds, uright=ur)
            try:
                (off_f, idx_f), (off_g, idx_g) = F.grid(), G.grid()
                assert np.array_equal(off_f, off_g) and np.array_equal(idx_f, idx_g)
                if len(k):
                    assert 0 < nv < len(k) and (ur > 0).sum() > 20
                    q, qd = _gated_queries(orbgpu_mod, k_un, desc, ur, 7 + f)
                    grid = orbgpu_mod.frame_grid(k_un, *bounds)
                    a = m.search_by_projection(orbgpu_mod.PROJ_BEST, q, qd, desc, k_un, grid, ur, min_xy=min_xy)
                    b = m.search_by_projection(orbgpu_mod.PROJ_BEST, q, qd, frame=F, use_uright=True)
                    c = m.search_by_projection(orbgpu_mod.PROJ_BEST, q, qd, desc, k_un, grid, None, min_xy=min_xy)
                    assert a[0] == b[0] > 0 and np.array_equal(a[1], b[1])
                    gated += int(not np.array_equal(a[1], c[1]))   # the gate changed the result: uright was read
            finally:
                G.close()
        assert gated > 0
        assert ext.results(0)[0].tobytes() == host[0][0].tobytes()   # the raw keypoints are not modified
        # without output arrays the handles are the same
        again = orbgpu_mod.Frame.from_batch_rgbd(ext, dist, dm, MBF, 3, ext.d_desc, ext.d_kps, ext.d_counts, cap,
                                                 bounds=bounds)
        try:
            for F, G in zip(frames, again):
                assert len(F) == len(G) and all(np.array_equal(x, y) for x, y in zip(F.grid(), G.grid()))
            k, desc = host[2]
            q, qd = _gated_queries(orbgpu_mod, _expected_un(orbgpu_mod, k), desc, got_ur[2 * cap:2 * cap + len(k)], 3)
            a = m.search_by_projection(orbgpu_mod.PROJ_BEST, q, qd, frame=frames[2], use_uright=True)
            b = m.search_by_projection(orbgpu_mod.PROJ_BEST, q, qd, frame=again[2], use_uright=True)
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
        finally:
            for F in again:
                F.close()
    finally:
        for F in frames:
            F.close()
        for b in bufs:
            b.close()


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_rgbd_mirror")


def _read_frame(buf, pos):
    n = struct.unpack_from("<i", buf, pos)[0]
    off = np.frombuffer(buf, np.int32, NCELL, pos + 4)
    ns = struct.unpack_from("<i", buf, pos + 4 + 4 * NCELL)[0]
    idx = np.frombuffer(buf, np.int32, ns, pos + 8 + 4 * NCELL)
    return (n, off, idx), pos + 8 + 4 * NCELL + 4 * ns


def test_cpp_and_python_mirrors(orbgpu_mod, L, m, extraction, mirror_bin, tmp_path):
    """The C++ program converts a BGR image (ColorImageView overload: keypoints, descriptors, mvImagePyramid[0]), runs
    ComputeStereoFromRGBD on one frame and ResidentFrame::FromBatchRGBD on the batch; the Python mirrors do the same."""
    from orbgpu.synth import synth_frame
    ext, host = extraction
    cap = ext.kp_cap
    depth = _depth_images()
    counts = np.array([len(host[f][0]) for f in range(3)], np.int32)
    k_all = np.zeros(3 * cap, orbgpu_mod.KP_DTYPE)
    d_all = np.zeros((3 * cap, 32), np.uint8)
    for f in range(3):
        k_all[f * cap:f * cap + counts[f]] = host[f][0]
        d_all[f * cap:f * cap + counts[f]] = host[f][1]
    bgr = np.stack([synth_frame(W, H, 20 + c) for c in range(3)], -1)
    src, dst = tmp_path / "case.bin", tmp_path / "results.bin"
    with open(src, "wb") as fh:
        fh.write(np.array(SMALL[:4] + SMALL[4], f32).tobytes())
        fh.write(np.array([W, H, 3, cap], np.int32).tobytes())
        fh.write(np.array([MBF, TUM], f32).tobytes())
        fh.write(counts.tobytes() + k_all.tobytes() + d_all.tobytes() + depth.tobytes() + bgr.tobytes())
    p = subprocess.run([mirror_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    buf = dst.read_bytes()

    # what the C-ABI gives
    gray = ref.to_gray(bgr, ref.COLOR_BGR)
    e1 = orbgpu_mod.ORBextractor(500, 1.2, 8, 20, 7)
    try:
        ck, cd = e1(gray)
        pk, pd = e1(bgr, color=orbgpu_mod.COLOR_BGR)          # Python mirror
        assert pk.tobytes() == ck.tobytes() and np.array_equal(pd, cd)
    finally:
        e1.close()
    assert np.array_equal(orbgpu_mod.to_gray_host(bgr, orbgpu_mod.COLOR_BGR), gray)
    dist = orbgpu_mod.distortion(*SMALL)
    bounds = tuple(orbgpu_mod.image_bounds(dist, W, H))
    un = [_expected_un(orbgpu_mod, host[f][0]) for f in range(3)]
    rg = [orbgpu_mod.stereo_from_rgbd_host(depth[f], TUM, host[f][0], un[f], MBF) for f in range(3)]

    # C++: the colour extraction
    pos = 0
    n = struct.unpack_from("<i", buf, pos)[0]
    assert n == len(ck) > 100
    assert buf[4:4 + 28 * n] == ck.tobytes() and buf[4 + 28 * n:4 + 60 * n] == cd.tobytes()
    pos = 4 + 60 * n
    assert buf[pos:pos + W * H] == gray.tobytes()
    pos += W * H
    # ComputeStereoFromRGBD of frame 0
    n0, nv0 = struct.unpack_from("<ii", buf, pos)
    assert n0 == counts[0] and nv0 == rg[0][2]
    pos += 8
    assert buf[pos:pos + 4 * n0] == rg[0][0].tobytes() and buf[pos + 4 * n0:pos + 8 * n0] == rg[0][1].tobytes()
    pos += 8 * n0
    # FromBatchRGBD: each frame's grid and flag, then the batch's uright / depth arrays
    for f in range(3):
        has_ur = struct.unpack_from("<i", buf, pos)[0]
        got, pos = _read_frame(buf, pos + 4)
        G = orbgpu_mod.Frame(m, host[f][1], un[f], bounds=bounds, uright=rg[f][0])
        try:
            off, idx = G.grid()
        finally:
            G.close()
        assert has_ur == 1 and got[0] == counts[f] and np.array_equal(got[1], off) and np.array_equal(got[2], idx), f
    ur = np.frombuffer(buf, f32, 3 * cap, pos)
    dep = np.frombuffer(buf, f32, 3 * cap, pos + 12 * cap)
    assert pos + 24 * cap == len(buf)
    for f in range(3):
        s = slice(f * cap, f * cap + counts[f])
        assert ur[s].tobytes() == rg[f][0].tobytes() and dep[s].tobytes() == rg[f][1].tobytes(), f

    # Python: BatchExtractor.stereo_from_rgbd over the extraction (no distortion: d_kps on both sides)
    bufs = [Dev(L, ext.h, a) for a in (depth, np.full(3 * cap, SENT, f32), np.full(3 * cap, SENT, f32),
                                       np.full(3, -5, np.int32))]
    d_map, d_ur, d_dep, d_nv = bufs
    try:
        dm = orbgpu_mod.depth_map(d_map.p, orbgpu_mod.DEPTH_U16, W, H, factor=TUM)
        ext.stereo_from_rgbd(dm, MBF, ext.d_kps, d_ur.p, d_dep.p, d_nv.p)
        ext.sync()
        g_ur, g_d, g_n = d_ur.get(f32), d_dep.get(f32), d_nv.get(np.int32)
        for f in range(3):
            w_ur, w_d, w_n = orbgpu_mod.stereo_from_rgbd_host(depth[f], TUM, host[f][0], host[f][0], MBF)
            s = slice(f * cap, f * cap + counts[f])
            assert g_ur[s].tobytes() == w_ur.tobytes() and g_d[s].tobytes() == w_d.tobytes() and g_n[f] == w_n
    finally:
        for b in bufs:
            b.close()
