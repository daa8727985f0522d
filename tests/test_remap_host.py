"""The CPU definitions of the stereo rectification (no GPU, no context): orb_remap_host against its known answers and the
int64 numpy model (remap_ref.py) over every fraction pair and over random maps thrown outside every side;
orb_rectify_maps_host against the float64 model; every argument check of the new entry points (all are made before the
context is touched, so the device forms are called here with a NULL context) with the outputs untouched; and
csrc/remap_def.h as a stand-alone program under ASan + UBSan (tests/cpp_remap/remap_host_test.cc)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import remap_ref as ref
from conftest import ROOT

f32 = np.float32
ARG = -1
SENT = 0xA5


@pytest.fixture(scope="module")
def L(orbgpu_mod):
    from orbgpu import _lib
    return _lib.lib()


def _refused(L, st):
    """ORB_ERR_ARG from the entry point's own check, not from the NULL context these tests pass."""
    msg = L.orb_last_error() or b""
    return st == ARG and b"NULL context" not in msg


def _row(orbgpu, src_row, mx, my=0.0):
    """One destination pixel of a one-row source."""
    src = np.asarray(src_row, np.uint8).reshape(1, -1)
    return int(orbgpu.remap_host(src, np.array([[mx]], f32), np.array([[my]], f32))[0, 0])


def _col(orbgpu, src_col, my):
    src = np.asarray(src_col, np.uint8).reshape(-1, 1)
    return int(orbgpu.remap_host(src, np.array([[0.0]], f32), np.array([[my]], f32))[0, 0])


def test_remap_known_answers(orbgpu_mod):
    rng = np.random.default_rng(1)
    S = rng.integers(1, 256, 9, dtype=np.uint8)
    S[0], S[8] = 201, 77        # odd ends: (S + 1) >> 1 differs from S >> 1
    sw = len(S)
    # the identity map returns the source
    img = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(7, dtype=f32), np.arange(9, dtype=f32), indexing="ij")
    assert np.array_equal(orbgpu_mod.remap_host(img, xx, yy), img)
    # x + 0.5: the rounded mean of two neighbours
    for x in range(sw - 1):
        assert _row(orbgpu_mod, S, x + 0.5) == (int(S[x]) + int(S[x + 1]) + 1) >> 1
    # the fraction rounds to nearest, ties to even: x + 1/64 is fraction 0.5 -> 0, x + 3/64 is 1.5 -> 2
    a, b = int(S[3]), int(S[4])
    assert _row(orbgpu_mod, S, 3 + 1 / 64) == a
    assert _row(orbgpu_mod, S, 3 + 3 / 64) == (30 * 32 * 32 * a + 2 * 32 * 32 * b + 16384) >> 15
    assert _row(orbgpu_mod, S, 3 + 3 / 64) != (31 * 32 * 32 * a + 1 * 32 * 32 * b + 16384) >> 15 or a == b
    # the borders, in x and in y
    for one in (_row, _col):
        at = lambda v: one(orbgpu_mod, S, v)
        assert at(-0.5) == (int(S[0]) + 1) >> 1 == 101
        assert at(sw - 1) == S[sw - 1]
        assert at(sw - 0.5) == (int(S[sw - 1]) + 1) >> 1 == 39
        for v in (float(sw), -1.0, 4e4, -4e4, 1e30, np.nan, np.inf, -np.inf):
            assert at(v) == 0, v
    # a position outside in y alone is 0 whatever x is
    assert _row(orbgpu_mod, S, 3.0, my=1.0) == 0 and _row(orbgpu_mod, S, 3.0, my=-1.0) == 0


def test_remap_all_fractions(orbgpu_mod):
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (6, 8), dtype=np.uint8)
    mx, my = ref.all_fractions_maps()
    ix, iy, fx, fy = ref.taps(mx, my)
    assert len(set(zip(fx.ravel().tolist(), fy.ravel().tolist()))) == 1024 and (ix == 3).all() and (iy == 2).all()
    assert np.array_equal(orbgpu_mod.remap_host(src, mx, my), ref.remap(src, mx, my))


@pytest.mark.parametrize("dw,dh,sw,sh", [(67, 35, 59, 41), (5, 3, 9, 4)])
def test_remap_random_cases(orbgpu_mod, L, dw, dh, sw, sh):
    rng = np.random.default_rng(dw)
    img = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    mx, my = ref.random_maps(dw, dh, sw, sh, seed=7 + dw)
    want = ref.remap(img, mx, my)
    ix, iy, _, _ = ref.taps(mx, my)
    # the case holds what it is meant to hold: taps beyond each side (the 15-pixel map has room for one or two throws
    # only), and most pixels inside
    outside = (ix < 0) | (ix >= sw) | (iy < 0) | (iy >= sh)
    assert outside.any() and not outside.all()
    if dw > 32:
        assert (ix < -1).any() and (ix >= sw).any() and (iy < -1).any() and (iy >= sh).any()
        assert ((ix >= 0) & (ix < sw - 1) & (iy >= 0) & (iy < sh - 1)).mean() > 0.7
    assert np.array_equal(orbgpu_mod.remap_host(img, mx, my), want)
    # odd strides on every side, bases at odd addresses: padding is neither read as pixels nor written
    for spad, dpad, mpad in ((1, 3, 4), (7, 1, 12)):
        ss, ds, ms = sw + spad, dw + dpad, 4 * dw + mpad
        src = np.full(1 + sh * ss, 0xEE, np.uint8)
        for y in range(sh):
            src[1 + y * ss:1 + y * ss + sw] = img[y]
        mbx, mby = np.full(dh * ms, 0xFF, np.uint8), np.full(dh * ms, 0xFF, np.uint8)   # (padding: NaN bit patterns)
        for y in range(dh):
            mbx[y * ms:y * ms + 4 * dw] = mx[y].view(np.uint8)
            mby[y * ms:y * ms + 4 * dw] = my[y].view(np.uint8)
        dst = np.full(3 + dh * ds, SENT, np.uint8)
        exp = dst.copy()
        for y in range(dh):
            exp[3 + y * ds:3 + y * ds + dw] = want[y]
        assert L.orb_remap_host(src.ctypes.data + 1, sw, sh, ss, mbx.ctypes.data, mby.ctypes.data, ms, dw, dh,
                                dst.ctypes.data + 3, ds) == 0
        assert np.array_equal(dst, exp), (spad, dpad, mpad)


def test_map_builder(orbgpu_mod, L):
    w, h = 40, 30
    K, _, _, _ = ref.small_calibration(w, h, 4)
    I = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    # D = 0, R = I, P33 = K: the model and the library agree bit for bit, and the maps are the pixel grid
    mx, my = orbgpu_mod.rectify_maps_host(K, [0.0] * 4, I, K, (w, h))
    rx, ry = ref.rectify_maps(K, [0.0] * 4, I, K, w, h)
    assert mx.tobytes() == rx.tobytes() and my.tobytes() == ry.tobytes()
    yy, xx = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    assert np.array_equal(mx, xx) and np.array_equal(my, yy)
    # a power-of-two camera makes every step exact: P33's cx shifted by an integer shifts the map by it
    K2 = [64.0, 0, 16.0, 0, 32.0, 8.0, 0, 0, 1.0]
    P2 = list(K2)
    P2[2] += 5.0
    sx, sy = orbgpu_mod.rectify_maps_host(K2, [0.0] * 4, I, P2, (w, h))
    assert np.array_equal(sx, xx - 5) and np.array_equal(sy, yy)
    # 4, 5 and 8 coefficients, a rotation, another rectified camera, a 3 x 4 P
    for ncoef in (4, 5, 8):
        K, D, R, P = ref.small_calibration(w, h, ncoef)
        P34 = np.concatenate([np.reshape(P, (3, 3)), [[-47.9], [0.0], [0.0]]], 1)
        mx, my = orbgpu_mod.rectify_maps_host(K, D, R, P34, (w, h))
        rx, ry = ref.rectify_maps(K, D, R, P, w, h)
        assert mx.tobytes() == rx.tobytes() and my.tobytes() == ry.tobytes(), ncoef
        assert np.abs(mx - xx).max() > 0.5 and np.abs(mx - xx).max() < 8      # distorted, mildly
    m8, _ = orbgpu_mod.rectify_maps_host(*ref.small_calibration(w, h, 8)[:3], ref.small_calibration(w, h, 8)[3], (w, h))
    m4, _ = orbgpu_mod.rectify_maps_host(*ref.small_calibration(w, h, 4)[:3], ref.small_calibration(w, h, 4)[3], (w, h))
    assert m8.tobytes() != m4.tobytes()                                     # k3..k6 are read
    # the sequential column sums are the definition: j * ir[0] gives other bits somewhere in a wider map
    K, D, R, P = ref.small_calibration(752, 8, 5)
    wx, _ = orbgpu_mod.rectify_maps_host(K, D, R, P, (752, 8))
    assert wx.tobytes() == ref.rectify_maps(K, D, R, P, 752, 8)[0].tobytes()

    # refusals: 12 and 14 coefficients, other counts, a singular P33 * R, NULL and misaligned arrays; outputs untouched
    out_x, out_y = np.full((h, w), 7, f32), np.full((h, w), 7, f32)
    Kd, Rd, Dd = (np.array(a, np.float64) for a in (K, R, list(D) + [0.0] * 9))
    sing, eye = np.array([1.0, 2, 3, 2, 4, 6, 0, 0, 1]), np.array(I, np.float64)   # (an exact zero determinant)

    def build(k=Kd, d=Dd, nd=5, r=Rd, p=Kd, ww=w, hh=h, ox=out_x.ctypes.data, oy=out_y.ctypes.data, ms=4 * w):
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.orb_rectify_maps_host(ptr(k), ptr(d), nd, ptr(r), ptr(p), ww, hh, ox, oy, ms)

    for kw in (dict(nd=12), dict(nd=14), dict(nd=0), dict(nd=3), dict(nd=6), dict(nd=-1), dict(p=sing, r=eye), dict(k=None),
               dict(d=None), dict(r=None), dict(p=None), dict(ox=None), dict(oy=None), dict(ww=-1), dict(hh=-1),
               dict(ww=4097, ms=4 * 4097), dict(hh=4097), dict(ms=4 * w - 4), dict(ms=4 * w + 2),
               dict(ox=out_x.ctypes.data + 2)):
        assert _refused(L, build(**kw)), kw
        assert (out_x == 7).all() and (out_y == 7).all(), kw
    assert build(ww=0) == 0 and build(hh=0, ox=None, oy=None) == 0 and (out_x == 7).all()
    assert build() == 0 and not (out_x == 7).any()


def test_remap_argument_errors(orbgpu_mod, L):
    w, h = 8, 4
    src = np.full(64 * 64, 1, np.uint8)
    dst = np.full(64 * 64, SENT, np.uint8)
    mx = np.zeros((h, w), f32)
    my = np.zeros((h, w), f32)
    S, D, MX, MY = src.ctypes.data, dst.ctypes.data, mx.ctypes.data, my.ctypes.data

    def host(s=S, sw=8, sh=4, ss=8, x=MX, y=MY, ms=32, dw=w, dh=h, d=D, ds=8):
        return L.orb_remap_host(s, sw, sh, ss, x, y, ms, dw, dh, d, ds)

    assert host() == 0 and (dst[:32] == 1).all()
    dst[:] = SENT
    for kw in (dict(s=None), dict(d=None), dict(x=None), dict(y=None), dict(sw=-1), dict(sh=-1), dict(dw=-1), dict(dh=-1),
               dict(ss=7), dict(ds=7), dict(ms=31), dict(ms=28), dict(ms=34), dict(x=MX + 1), dict(y=MY + 2),
               dict(sw=4097, ss=4097), dict(sh=4097), dict(dw=4097, ms=4 * 4097, ds=4097), dict(dh=4097)):
        assert _refused(L, host(**kw)), kw
        assert (dst == SENT).all(), kw
    assert host(dw=0) == 0 and host(dh=0, x=None, y=None, d=None) == 0 and (dst == SENT).all()
    assert host(sw=0, s=None) == 0 and (dst[:32] == 0).all()      # an empty source: every tap is outside
    dst[:] = SENT

    # orb_rectify_create checks its maps before it touches the context (NULL here)
    out = ctypes.c_void_p(7)

    def create(dw=w, dh=h, x=MX, y=MY, ms=32, o=ctypes.byref(out)):
        return L.orb_rectify_create(None, dw, dh, x, y, ms, o)

    for kw in (dict(dw=-1), dict(dh=-1), dict(dw=4097, ms=4 * 4097), dict(dh=4097), dict(x=None), dict(y=None),
               dict(ms=28), dict(ms=34), dict(x=MX + 2), dict(y=MY + 1), dict(o=None)):
        assert _refused(L, create(**kw)), kw
        assert out.value == 7, kw
    assert create() == ARG and not _refused(L, ARG) and out.value == 7      # (the NULL context)
    w_, h_ = ctypes.c_int(7), ctypes.c_int(7)
    assert _refused(L, L.orb_rectify_size(None, ctypes.byref(w_), ctypes.byref(h_))) and w_.value == 7
    L.orb_rectify_destroy(None)

    # the handle-taking calls refuse a missing handle before anything else; what a real handle refuses is in
    # tests/test_gpu_remap.py
    kps = np.full(8, 7, orbgpu_mod.KP_DTYPE)
    desc = np.full((8, 32), 7, np.uint8)
    n = ctypes.c_int(7)
    null2 = (ctypes.c_void_p * 2)(None, None)
    assert _refused(L, L.orb_remap_device(None, 0, null2, S, 2, 8, 4, 32, 8, D, 32, 8))
    assert _refused(L, L.orb_remap_device(None, -1, null2, S, 2, 8, 4, 32, 8, D, 32, 8))
    assert _refused(L, L.orb_remap_device(None, 17, null2, S, 2, 8, 4, 32, 8, D, 32, 8))
    assert _refused(L, L.orb_remap_device(None, 2, None, S, 2, 8, 4, 32, 8, D, 32, 8))
    assert _refused(L, L.orb_remap_device(None, 2, null2, S, 2, 8, 4, 32, 8, D, 32, 8))
    assert _refused(L, L.orb_remap(None, None, S, 8, 4, 8, D, 8))
    assert _refused(L, L.orb_extract_rectified(None, None, S, 8, 4, 8, kps.ctypes.data, 8, ctypes.byref(n),
                                               desc.ctypes.data))
    assert (dst == SENT).all() and n.value == 7 and (desc == 7).all()


def test_stereo_constructor_argument_errors(orbgpu_mod, L):
    """orb_frames_create_from_batch_stereo: what it refuses before it touches the context (NULL here)."""
    from orbgpu._lib import OrbDistortion
    dist = OrbDistortion()
    dist.fx, dist.fy, dist.cx, dist.cy = 350.0, 351.0, 160.0, 120.0
    bad_dist = OrbDistortion()
    bad_dist.fx, bad_dist.fy = 0.0, 1.0
    P = np.zeros(64, np.uint8).ctypes.data
    out = (ctypes.c_void_p * 2)(7, 7)

    def ctor(d=dist, npairs=2, mb=0.1, mbf=40.0, desc=P, raw=P, cnt=P, cap=10, inv_w=0.2, min_x=0.0, o=out):
        return L.orb_frames_create_from_batch_stereo(None, None if d is None else ctypes.byref(d), npairs, mb, mbf, desc,
                                                     raw, cnt, cap, min_x, 0.0, inv_w, 0.2, None, None, o)

    for kw in (dict(d=None), dict(d=bad_dist), dict(npairs=-1), dict(npairs=32768), dict(cap=0), dict(cap=1 << 30),
               dict(mb=float("nan")), dict(mbf=float("inf")), dict(desc=None), dict(raw=None), dict(cnt=None),
               dict(o=None), dict(inv_w=0.0), dict(inv_w=float("nan")), dict(min_x=float("inf"))):
        assert _refused(L, ctor(**kw)), kw
        assert out[0] == 7 and out[1] == 7, kw
    assert ctor(npairs=0, desc=None, raw=None, cnt=None, o=None) == 0
    assert ctor() == ARG and not _refused(L, ARG) and out[0] == 7          # (the NULL context)


def test_remap_definitions_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "remap_host_test")
    src = os.path.join(ROOT, "tests", "cpp_remap", "remap_host_test.cc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "remap_def OK" in r.stdout, r.stdout + r.stderr
