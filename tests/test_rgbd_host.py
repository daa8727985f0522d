"""The CPU definitions of the colour and RGB-D entry points (no GPU, no context): orb_to_gray_host against the integer
formula's known answers and across layouts, orb_stereo_from_rgbd_host against the np.float32 restatement on the
planted case, and every argument check of the new entry points (all are made before the context is touched, so the
device forms are called here with a NULL context) with the outputs untouched."""
import ctypes

import numpy as np
import pytest

import rgbd_ref as ref

f32 = np.float32
ARG = -1
# (R, G, B) whose weighted sum is 8191 / 8192 mod 16384: the largest sum that still rounds down, the smallest that
# rounds up.  Found by _search_rounding_triples(), hard-coded.
ROUND_DOWN = ((142, 69, 224), 108)   # 4899*142 + 9617*69 + 1868*224 = 1777663 = 108 * 16384 + 8191
ROUND_UP = ((153, 209, 255), 198)    # 4899*153 + 9617*209 + 1868*255 = 3235840 = 197 * 16384 + 8192


def _search_rounding_triples():
    r, g, b = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    s = 4899 * r + 9617 * g + 1868 * b
    out = []
    for t in (8191, 8192):
        i = np.argwhere((s % 16384 == t) & (r > 50) & (g > 50) & (b > 50) & (r != b))
        out.append(tuple(int(v) for v in i[len(i) // 2]))
    return out


@pytest.fixture(scope="module")
def L(orbgpu_mod):
    from orbgpu import _lib
    return _lib.lib()


def _refused(L, st):
    """ORB_ERR_ARG from the entry point's own check, not from the NULL context these tests pass."""
    msg = L.orb_last_error() or b""
    return st == ARG and b"NULL context" not in msg


def _gray1(orbgpu, rgb, color=ref.COLOR_RGB):
    px = np.array(rgb, np.uint8).reshape(1, 1, 3)
    if color == ref.COLOR_BGR:
        px = px[..., ::-1]
    return int(orbgpu.to_gray_host(px, color)[0, 0])


def test_gray_known_answers(orbgpu_mod):
    g = lambda *rgb: _gray1(orbgpu_mod, rgb)
    assert g(255, 255, 255) == 255 and g(0, 0, 0) == 0
    assert (g(255, 0, 0), g(0, 255, 0), g(0, 0, 255)) == (76, 150, 29)
    for (rgb, want), rem in ((ROUND_DOWN, 8191), (ROUND_UP, 8192)):
        s = 4899 * rgb[0] + 9617 * rgb[1] + 1868 * rgb[2]
        assert s % 16384 == rem and want == (s + 8192) >> 14
        assert g(*rgb) == want and _gray1(orbgpu_mod, rgb, ref.COLOR_BGR) == want
    assert ROUND_DOWN[1] == (4899 * 142 + 9617 * 69 + 1868 * 224) >> 14          # rounds down: the plain quotient
    assert ROUND_UP[1] == ((4899 * 153 + 9617 * 209 + 1868 * 255) >> 14) + 1     # rounds up: one above it


def test_hard_coded_triples_are_what_the_search_finds():
    assert _search_rounding_triples() == [ROUND_DOWN[0], ROUND_UP[0]]


def _layouts(rgb, alpha):
    """The same colours in the four layouts."""
    bgr = rgb[..., ::-1]
    a = alpha[..., None]
    return {ref.COLOR_RGB: rgb, ref.COLOR_BGR: bgr, ref.COLOR_RGBA: np.concatenate([rgb, a], -1),
            ref.COLOR_BGRA: np.concatenate([bgr, a], -1)}


def test_to_gray_host_across_layouts(orbgpu_mod, L):
    rng = np.random.default_rng(3)
    h, w = 7, 13
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = ref.gray_rgb(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    for alpha in (np.zeros((h, w), np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)):   # alpha is ignored
        for code, img in _layouts(rgb, alpha).items():
            assert np.array_equal(orbgpu_mod.to_gray_host(np.ascontiguousarray(img), code), want), code
            assert np.array_equal(ref.to_gray(img, code), want)
    # strides with padding on both sides, bases at odd addresses: the padding is neither read as pixels nor written
    for code, img in _layouts(rgb, np.full((h, w), 9, np.uint8)).items():
        ch = img.shape[2]
        for spad, dpad in ((0, 0), (1, 3), (7, 1)):
            ss, ds = w * ch + spad, w + dpad
            src = np.full(1 + h * ss, 0xEE, np.uint8)
            for y in range(h):
                src[1 + y * ss: 1 + y * ss + w * ch] = img[y].ravel()
            dst = np.full(3 + h * ds, 0xA5, np.uint8)
            exp = dst.copy()
            for y in range(h):
                exp[3 + y * ds: 3 + y * ds + w] = want[y]
            assert L.orb_to_gray_host(code, src.ctypes.data + 1, w, h, ss, dst.ctypes.data + 3, ds) == 0
            assert np.array_equal(dst, exp), (code, spad, dpad)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("factor", [f32(1.0) / f32(5000.0), f32(1.0)])
def test_stereo_from_rgbd_host_equals_the_reference(orbgpu_mod, kind, factor):
    m = ref.planted_map(kind)
    k, ku = ref.planted_keypoints(200)
    mbf = f32(40.0)
    want_ur, want_d, want_n, outside = ref.stereo_from_rgbd(m, factor, k, ku, mbf)
    assert not outside.any()
    ur, d, n = orbgpu_mod.stereo_from_rgbd_host(m, factor, k, ku, mbf)
    assert ur.tobytes() == want_ur.tobytes() and d.tobytes() == want_d.tobytes() and n == want_n
    # the case holds what it is meant to hold
    if kind == "f32":
        sp = np.array(ref.SPECIAL_F32, f32)
        fails = ~(sp * factor > 0)                      # 0, -0, -1, NaN, -inf (and what underflows to 0)
        assert fails[:4].all() and fails[11] and not fails[4]
        assert (d[:12][fails] == -1).all() and (ur[:12][fails] == -1).all()
        assert np.isinf(d[4]) and ur[4] == ku["x"][4]   # +inf passes: uright = kpU.x
        if factor == 1:
            assert 0 < d[5] < np.finfo(f32).tiny        # the subnormal passes d > 0
    else:
        assert d[0] == -1 and ur[0] == -1 and d[1] == f32(1) * factor and d[2] == f32(65535) * factor
    assert 20 < n < 200 and int(np.trunc(k["x"][12])) == 10 and k["x"][12] == f32(10.999)
    assert d[12] == f32(f32(m[3, 10]) * factor) or (d[12] == -1 and not f32(m[3, 10]) * factor > 0)
    assert d[13] == (f32(f32(m[0, 0]) * factor) if f32(m[0, 0]) * factor > 0 else -1)
    # a row stride larger than the row gives the same bytes
    wide = np.zeros((m.shape[0], m.shape[1] + 5), m.dtype)
    wide[:, :m.shape[1]] = m
    ur2, d2, n2 = orbgpu_mod.stereo_from_rgbd_host(wide[:, :m.shape[1]], factor, k, ku, mbf)
    assert ur2.tobytes() == want_ur.tobytes() and d2.tobytes() == want_d.tobytes() and n2 == want_n
    # the wrong array on either side would show
    assert ref.stereo_from_rgbd(m, factor, ku, ku, mbf)[1].tobytes() != want_d.tobytes()
    assert ref.stereo_from_rgbd(m, factor, k, k, mbf)[0].tobytes() != want_ur.tobytes()


def test_to_gray_argument_errors(orbgpu_mod, L):
    src = np.full(64 * 64 * 4, 1, np.uint8)
    dst = np.full(64 * 64, 0xA5, np.uint8)
    S, D = src.ctypes.data, dst.ctypes.data
    host = lambda code=0, s=S, w=8, h=4, ss=24, d=D, ds=8: L.orb_to_gray_host(code, s, w, h, ss, d, ds)
    assert host() == 0
    dst[:] = 0xA5
    for kw in (dict(code=4), dict(code=-1), dict(s=None), dict(d=None), dict(w=-1), dict(h=-1), dict(ss=23), dict(ds=7),
               dict(code=2, ss=31), dict(w=4097, ss=3 * 4097, ds=4097), dict(h=4097)):
        assert _refused(L, host(**kw)), kw
        assert (dst == 0xA5).all(), kw
    assert host(w=0) == 0 and host(h=0) == 0 and host(w=0, s=None, d=None) == 0 and (dst == 0xA5).all()

    def dev(code=0, s=S, n=2, w=8, h=4, sfp=96, srs=24, d=D, dfp=32, drs=8):
        return L.orb_to_gray_device(None, code, s, n, w, h, sfp, srs, d, dfp, drs)

    for kw in (dict(code=7), dict(s=None), dict(d=None), dict(n=-1), dict(w=-1), dict(h=-2), dict(srs=23), dict(drs=7),
               dict(w=4097, srs=3 * 4097, drs=4097, sfp=1 << 20, dfp=1 << 20), dict(h=4097, sfp=1 << 20, dfp=1 << 20),
               dict(sfp=95), dict(dfp=31)):
        assert _refused(L, dev(**kw)), kw
    assert dev(n=0, s=None, d=None) == 0 and dev(w=0) == 0      # nothing to convert: ORB_OK without a context
    assert dev(n=1, sfp=0, dfp=0) == ARG and not _refused(L, ARG)   # one frame: the pitches are not read (NULL context)

    kps = np.full(8, 7, orbgpu_mod.KP_DTYPE)
    desc = np.full((8, 32), 7, np.uint8)
    n = ctypes.c_int(7)

    def col(code=0, s=S, w=8, h=4, ss=24):
        return L.orb_extract_color(None, code, s, w, h, ss, kps.ctypes.data, 8, ctypes.byref(n), desc.ctypes.data)

    for kw in (dict(code=4), dict(w=-1), dict(h=-1), dict(ss=23), dict(code=3, ss=31), dict(w=4097, ss=3 * 4097),
               dict(h=4097)):
        assert _refused(L, col(**kw)), kw
        assert n.value == 7 and (desc == 7).all() and kps.tobytes() == np.full(8, 7, orbgpu_mod.KP_DTYPE).tobytes()


def test_rgbd_argument_errors(orbgpu_mod, L):
    from orbgpu._lib import OrbDepthMap, OrbDistortion
    m = ref.planted_map("u16")
    k, ku = ref.planted_keypoints(20)
    ur = np.full(20, 7, f32)
    dep = np.full(20, 7, f32)
    nv = ctypes.c_int(7)

    def dmap(data=m.ctypes.data, type=0, w=ref.MAP_W, h=ref.MAP_H, rs=2 * ref.MAP_W, fp=2 * ref.MAP_W * ref.MAP_H,
             factor=0.0002):
        return OrbDepthMap(data, type, w, h, rs, fp, factor)

    def host(mp=None, mbf=40.0, n=20, kps=k, kun=ku, o_ur=ur, o_d=dep, null_map=False):
        mp = mp or dmap()
        return L.orb_stereo_from_rgbd_host(None if null_map else ctypes.byref(mp), mbf, n,
                                           None if kps is None else kps.ctypes.data,
                                           None if kun is None else kun.ctypes.data,
                                           None if o_ur is None else o_ur.ctypes.data,
                                           None if o_d is None else o_d.ctypes.data, ctypes.byref(nv))

    assert host() == 0 and nv.value > 0
    ur[:] = 7
    dep[:] = 7
    nv.value = 7
    k_out, k_nan, k_inf, k_neg = k.copy(), k.copy(), k.copy(), k.copy()
    k_out["x"][19] = ref.MAP_W            # the LAST keypoint: nothing before it may have been written
    k_nan["y"][19] = np.nan
    k_inf["x"][19] = np.inf
    k_neg["y"][19] = -1.0
    bad_maps = (dmap(type=2), dmap(type=-1), dmap(factor=float("nan")), dmap(factor=float("inf")), dmap(w=-1),
                dmap(h=-1), dmap(w=4097, rs=2 * 4097), dmap(h=4097), dmap(rs=2 * ref.MAP_W - 1),
                dmap(type=1, rs=4 * ref.MAP_W - 4), dmap(data=None), dmap(data=m.ctypes.data + 1),
                dmap(rs=2 * ref.MAP_W + 1))
    cases = [dict(mp=b) for b in bad_maps] + [
        dict(null_map=True), dict(mbf=float("nan")), dict(mbf=float("-inf")), dict(n=-1), dict(kps=None),
        dict(kun=None), dict(o_ur=None), dict(o_d=None), dict(kps=k_out), dict(kps=k_nan), dict(kps=k_inf),
        dict(kps=k_neg)]
    for kw in cases:
        assert _refused(L, host(**kw)), kw
        assert (ur == 7).all() and (dep == 7).all() and nv.value == 7, kw
    assert host(n=0, kps=None, kun=None, o_ur=None, o_d=None) == 0 and nv.value == 0

    # the device forms check before they touch the context (NULL here); pointers are never dereferenced
    P = m.ctypes.data

    def dev(mp=None, mbf=40.0, nf=2, raw=P, un=P, cnt=P, cap=10, o_ur=P, o_d=P, null_map=False):
        mp = mp or dmap()
        return L.orb_stereo_from_rgbd_device(None, None if null_map else ctypes.byref(mp), mbf, nf, raw, un, cnt, cap,
                                             o_ur, o_d, None)

    dev_cases = [dict(mp=b) for b in bad_maps] + [
        dict(null_map=True), dict(mbf=float("inf")), dict(nf=-1), dict(cap=0), dict(nf=65536), dict(raw=None),
        dict(un=None), dict(cnt=None), dict(o_ur=None), dict(o_d=None), dict(mp=dmap(fp=2 * ref.MAP_W * ref.MAP_H - 2)),
        dict(mp=dmap(fp=2 * ref.MAP_W * ref.MAP_H + 1))]
    for kw in dev_cases:
        assert _refused(L, dev(**kw)), kw
    assert dev(nf=0, raw=None, un=None, cnt=None, o_ur=None, o_d=None) == 0

    dist = OrbDistortion()
    dist.fx, dist.fy, dist.cx, dist.cy = 350.0, 351.0, 160.0, 120.0
    out = (ctypes.c_void_p * 2)(7, 7)

    def ctor(mp=None, mbf=40.0, nf=2, desc=P, raw=P, cnt=P, cap=10, inv_w=0.2, d=dist, o=out, null_map=False):
        mp = mp or dmap()
        return L.orb_frames_create_from_batch_rgbd(None, None if d is None else ctypes.byref(d),
                                                   None if null_map else ctypes.byref(mp), mbf, nf, desc, raw, cnt, cap,
                                                   0.0, 0.0, inv_w, 0.2, None, None, o)

    bad_dist = OrbDistortion()
    bad_dist.fx, bad_dist.fy = 0.0, 1.0
    ctor_cases = [dict(mp=b) for b in bad_maps] + [
        dict(null_map=True), dict(mbf=float("nan")), dict(nf=-1), dict(cap=0), dict(desc=None), dict(raw=None),
        dict(cnt=None), dict(o=None), dict(inv_w=0.0), dict(inv_w=float("nan")), dict(d=None), dict(d=bad_dist)]
    for kw in ctor_cases:
        assert _refused(L, ctor(**kw)), kw
        assert out[0] == 7 and out[1] == 7, kw
    assert ctor(nf=0, desc=None, raw=None, cnt=None, o=None) == 0
