"""k_remap on the GPU, byte for byte against the CPU definition orb_remap_host (itself checked against the int64 numpy
model in test_remap_host.py): the widths, alignments and strides at which the kernel takes its byte path, every fraction
pair, maps thrown outside every side, the index arithmetic of a 4096-wide and a 4096-high frame, the batch forms with
one and two maps, and the host-image forms orb_remap and orb_extract_rectified with the stereo search behind them."""
import ctypes

import numpy as np
import pytest

import remap_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT = 0xA5
ARG = -1


@pytest.fixture(scope="module")
def L(orbgpu_mod):
    from orbgpu import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def ctx(orbgpu_mod):
    c = orbgpu_mod._Ctx(1000, 1.2, 8, 20, 7, 0)
    yield c
    c.close()


class Dev:
    """A device allocation of the context, freed on close."""

    def __init__(self, L, ctx, nbytes):
        self.L, self.ctx, self.n = L, ctx, nbytes
        self.p = L.orb_device_alloc(ctx.h, nbytes)
        assert self.p

    def put(self, a, off=0):
        a = np.ascontiguousarray(a)
        assert off + a.nbytes <= self.n
        assert self.L.orb_memcpy_h2d(self.ctx.h, self.p + off, a.ctypes.data, a.nbytes) == 0

    def get(self, nbytes=None, off=0):
        out = np.zeros(self.n - off if nbytes is None else nbytes, np.uint8)
        assert self.L.orb_memcpy_d2h(self.ctx.h, out.ctypes.data, self.p + off, out.nbytes) == 0
        return out

    def close(self):
        self.L.orb_device_free(self.ctx.h, self.p)


def _remap_batch(orbgpu, L, ctx, src, dst, rects, imgs, want, so=0, do=0, spad=0, dpad=0, sgap=0, dgap=0):
    """imgs (n, sh, sw) laid out at src.p + so with row stride sw + spad and frame pitch sh * stride + sgap, remapped
    into dst.p + do likewise; the whole destination buffer must equal `want` (n, dh, dw) inside the rows and the
    sentinel everywhere else."""
    n, sh, sw = imgs.shape
    _, dh, dw = want.shape
    srs, drs = sw + spad, dw + dpad
    sfp, dfp = sh * srs + sgap, dh * drs + dgap
    s = np.full(so + n * sfp + 8, 0xEE, np.uint8)
    exp = np.full(do + n * dfp + 16, SENT, np.uint8)
    for f in range(n):
        for y in range(sh):
            o = so + f * sfp + y * srs
            s[o:o + sw] = imgs[f, y]
        for y in range(dh):
            o = do + f * dfp + y * drs
            exp[o:o + dw] = want[f, y]
    src.put(s)
    dst.put(np.full(len(exp), SENT, np.uint8))
    orbgpu.remap_device(ctx, rects, src.p + so, n, sw, sh, sfp, srs, dst.p + do, dfp, drs)
    assert L.orb_sync(ctx.h) == 0
    return np.array_equal(dst.get(len(exp)), exp)


def test_widths_alignments_strides(orbgpu_mod, L, ctx):
    """dw in {1, 3, 4, 5, 63, 64, 65, 67} x dh = 3 from a source of another size, bases offset by 0..3 bytes on either
    side, row strides of w, w + 1, w + 7: the destination equals the host definition's and every byte of its padding,
    before its base and past its end keeps the sentinel.  The maps throw a tenth of the pixels outside."""
    dh, sh = 3, 5
    src, dst = Dev(L, ctx, 1 << 12), Dev(L, ctx, 1 << 12)
    odd = 0
    try:
        for dw in (1, 3, 4, 5, 63, 64, 65, 67):
            sw = dw + 6
            rng = np.random.default_rng(50 + dw)
            img = rng.integers(0, 256, (1, sh, sw), dtype=np.uint8)
            mx, my = ref.random_maps(dw, dh, sw, sh, seed=dw)
            want = orbgpu_mod.remap_host(img[0], mx, my)[None]
            assert np.array_equal(want[0], ref.remap(img[0], mx, my))
            rect = orbgpu_mod.Rectifier(ctx, mx, my)
            try:
                assert rect.size == (dw, dh)
                for pad in (0, 1, 7):
                    odd += (dw + pad) % 4 != 0
                    for so in range(4):
                        for do in range(4):
                            assert _remap_batch(orbgpu_mod, L, ctx, src, dst, [rect], img, want, so, do, pad, pad), \
                                (dw, pad, so, do)
            finally:
                rect.close()
        assert odd > 12
    finally:
        src.close()
        dst.close()


def test_all_fractions_and_thrown_outside(orbgpu_mod, L, ctx):
    src, dst = Dev(L, ctx, 1 << 14), Dev(L, ctx, 1 << 14)
    try:
        rng = np.random.default_rng(2)
        img = rng.integers(0, 256, (1, 6, 8), dtype=np.uint8)
        mx, my = ref.all_fractions_maps()
        rect = orbgpu_mod.Rectifier(ctx, mx, my)
        try:
            assert _remap_batch(orbgpu_mod, L, ctx, src, dst, [rect], img, ref.remap(img[0], mx, my)[None])
        finally:
            rect.close()
        # 67 x 35 from 59 x 41: beyond all four sides, across the corners, positions no short or int holds
        img = rng.integers(1, 256, (1, 41, 59), dtype=np.uint8)
        mx, my = ref.random_maps(67, 35, 59, 41, seed=74)
        ix, iy, _, _ = ref.taps(mx, my)
        assert (ix < -1).any() and (ix >= 59).any() and (iy < -1).any() and (iy >= 41).any()
        assert ((ix >= 59) & (iy < 0)).any() and ((ix < 0) & (iy >= 41)).any()        # corners
        assert (ix == -1).any() and (iy == -1).any() and (ix == 58).any() and (iy == 40).any()   # half-outside taps
        want = orbgpu_mod.remap_host(img[0], mx, my)
        assert np.array_equal(want, ref.remap(img[0], mx, my))
        rect = orbgpu_mod.Rectifier(ctx, mx, my)
        try:
            assert _remap_batch(orbgpu_mod, L, ctx, src, dst, [rect], img, want[None], 1, 3, 5, 2)
            # an empty source reads 0 everywhere
            st = L.orb_remap_device(ctx.h, 1, (ctypes.c_void_p * 1)(rect.h), None, 1, 0, 0, 0, 0, dst.p, 0, 67)
            assert st == 0 and L.orb_sync(ctx.h) == 0 and not dst.get(67 * 35).any()
        finally:
            rect.close()
    finally:
        src.close()
        dst.close()


@pytest.mark.parametrize("dw,dh", [(4096, 2), (2, 4096)])
def test_longest_sides(orbgpu_mod, L, ctx, dw, dh):
    """One 4096 x 2 and one 2 x 4096 frame from a source of the transposed size: the index arithmetic at the limit."""
    sw, sh = dh + 1, dw + 1
    sw, sh = min(sw, 4096), min(sh, 4096)
    rng = np.random.default_rng(dw)
    img = rng.integers(0, 256, (1, sh, sw), dtype=np.uint8)
    mx, my = ref.random_maps(dw, dh, sw, sh, seed=dh)
    want = orbgpu_mod.remap_host(img[0], mx, my)
    assert np.array_equal(want, ref.remap(img[0], mx, my))
    src, dst = Dev(L, ctx, sw * sh + 64 + 3 * sh), Dev(L, ctx, (dw + 3) * dh + 64)
    rect = orbgpu_mod.Rectifier(ctx, mx, my)
    try:
        assert _remap_batch(orbgpu_mod, L, ctx, src, dst, [rect], img, want[None], 0, 0, 0, 0)
        assert _remap_batch(orbgpu_mod, L, ctx, src, dst, [rect], img, want[None], 1, 2, 3, 3)
    finally:
        rect.close()
        src.close()
        dst.close()


def test_batch_forms(orbgpu_mod, L, ctx):
    """nmaps = 1 with 3 and with 9 frames, nmaps = 2 with 5 frames whose left and right maps differ, frame pitches
    larger than a frame: every frame equals the host definition with its own map."""
    dw, dh, sw, sh = 37, 9, 41, 11
    rng = np.random.default_rng(9)
    maps = [ref.random_maps(dw, dh, sw, sh, seed=s) for s in (1, 2)]
    assert not np.array_equal(maps[0][0], maps[1][0])
    rects = [orbgpu_mod.Rectifier(ctx, mx, my) for mx, my in maps]
    src, dst = Dev(L, ctx, 1 << 14), Dev(L, ctx, 1 << 14)
    try:
        for nmaps, n in ((1, 3), (1, 9), (2, 5), (2, 2), (2, 1)):
            imgs = rng.integers(0, 256, (n, sh, sw), dtype=np.uint8)
            want = np.stack([orbgpu_mod.remap_host(imgs[f], *maps[f % nmaps]) for f in range(n)])
            if nmaps == 2 and n > 1:
                assert not np.array_equal(want[1], orbgpu_mod.remap_host(imgs[1], *maps[0]))   # the map matters
            assert _remap_batch(orbgpu_mod, L, ctx, src, dst, rects[:nmaps], imgs, want, 0, 0, 3, 1, sgap=13, dgap=22), \
                (nmaps, n)
            assert _remap_batch(orbgpu_mod, L, ctx, src, dst, rects[:nmaps], imgs, want, 2, 1, 0, 0), (nmaps, n)
    finally:
        for r in rects:
            r.close()
        src.close()
        dst.close()


# a 160 x 120 image holds four pyramid levels of the extractor (a level needs 62 pixels a side)
LEVELS = 4


def test_remap_and_extract_rectified(orbgpu_mod):
    w, h = 160, 120
    (rawL, mxL, myL), (rawR, mxR, myR) = ref.raw_pair(orbgpu_mod, w, h, 5)
    rectL_img, rectR_img = orbgpu_mod.remap_host(rawL, mxL, myL), orbgpu_mod.remap_host(rawR, mxR, myR)
    assert not np.array_equal(rectL_img, rawL)
    el, er = orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7), orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7)
    pl, pr = orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7), orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7)
    RL, RR = orbgpu_mod.Rectifier(el, mxL, myL), orbgpu_mod.Rectifier(er, mxR, myR)
    try:
        # orb_remap: a host image in, the rectified host image out; rows with padding on the way in
        assert np.array_equal(RL.remap(rawL), rectL_img) and np.array_equal(RR(rawR), rectR_img)
        wide = np.zeros((h, w + 5), np.uint8)
        wide[:, :w] = rawL
        assert np.array_equal(RL.remap(wide[:, :w]), rectL_img)
        # a raw image of another size than the maps
        crop = rawL[3:h - 2, 1:w - 7]
        assert np.array_equal(RL.remap(crop), orbgpu_mod.remap_host(crop, mxL, myL))
        # orb_extract_rectified: orb_extract on the host definition's output
        kl, dl = el(rawL, rectify=RL)
        lvl0 = el.mvImagePyramid[0]
        kr, dr = er(rawR, rectify=RR)
        ql, qdl = pl(rectL_img)
        qr, qdr = pr(rectR_img)
        assert len(kl) > 50 and len(kr) > 50
        assert kl.tobytes() == ql.tobytes() and np.array_equal(dl, qdl)
        assert kr.tobytes() == qr.tobytes() and np.array_equal(dr, qdr)
        assert np.array_equal(lvl0, rectL_img)
        for a, b in zip(el.mvImagePyramid, pl.mvImagePyramid):
            assert np.array_equal(a, b)
        # the two contexts are valid left / right arguments of the stereo search
        u1, d1, n1 = orbgpu_mod.compute_stereo_matches(el, er, kl, dl, kr, dr, 0.1, 0.1 * 90.0)
        u2, d2, n2 = orbgpu_mod.compute_stereo_matches(pl, pr, ql, qdl, qr, qdr, 0.1, 0.1 * 90.0)
        assert n1 == n2 > 5 and u1.tobytes() == u2.tobytes() and d1.tobytes() == d2.tobytes()
        # an empty image leaves the outputs as given
        assert el(np.zeros((0, 0), np.uint8), keypoints="k", descriptors="d", rectify=RL) == ("k", "d")
    finally:
        RL.close()
        RR.close()
        for e in (el, er, pl, pr):
            e.close()


def _refused(L, st):
    msg = L.orb_last_error() or b""
    return st == ARG and b"NULL context" not in msg


def test_argument_errors_with_handles(orbgpu_mod, L, ctx):
    """Every refusal of the handle-taking calls: ORB_ERR_ARG, the destination and the outputs untouched."""
    w, h = 8, 4
    mx, my = np.zeros((h, w), f32), np.zeros((h, w), f32)
    A, B = orbgpu_mod.Rectifier(ctx, mx, my), orbgpu_mod.Rectifier(ctx, mx[:, :4], my[:, :4])
    E = orbgpu_mod.Rectifier(ctx, np.zeros((0, 0), f32), np.zeros((0, 0), f32))
    src, dst = Dev(L, ctx, 4096), Dev(L, ctx, 4096)
    try:
        assert E.size == (0, 0)
        src.put(np.zeros(4096, np.uint8))
        dst.put(np.full(4096, SENT, np.uint8))
        hs = lambda *r: (ctypes.c_void_p * len(r))(*[x.h if x is not None else None for x in r])

        def dev(maps=hs(A, A), nmaps=2, s=src.p, n=2, sw=8, sh=4, sfp=32, srs=8, d=dst.p, dfp=32, drs=8):
            return L.orb_remap_device(ctx.h, nmaps, maps, s, n, sw, sh, sfp, srs, d, dfp, drs)

        for kw in (dict(nmaps=0), dict(nmaps=-2), dict(nmaps=17), dict(maps=None), dict(maps=hs(A, None)),
                   dict(maps=hs(A, B)), dict(s=None), dict(d=None), dict(n=-1), dict(sw=-1), dict(sh=-1),
                   dict(sw=4097, srs=4097, sfp=1 << 20), dict(sh=4097, sfp=1 << 20), dict(srs=7), dict(drs=7),
                   dict(sfp=31), dict(dfp=31)):
            assert _refused(L, dev(**kw)), kw
        assert dev(n=0, s=None, d=None) == 0 and dev(maps=hs(E), nmaps=1, s=None, d=None) == 0
        assert dev(n=1, sfp=0, dfp=0) == 0                      # one frame: the pitches are not read
        assert L.orb_sync(ctx.h) == 0
        got = dst.get()
        assert (got[:32] == 0).all() and (got[32:] == SENT).all()   # (only that last call wrote: src is zero-mapped)

        host_src = np.full(64, 9, np.uint8)
        host_dst = np.full(64, SENT, np.uint8)

        def one(r=A.h, s=host_src.ctypes.data, sw=8, sh=4, ss=8, d=host_dst.ctypes.data, ds=8):
            return L.orb_remap(ctx.h, r, s, sw, sh, ss, d, ds)

        for kw in (dict(r=None), dict(s=None), dict(d=None), dict(sw=-1), dict(sh=-1), dict(ss=7), dict(ds=7),
                   dict(sw=4097, ss=4097), dict(sh=4097)):
            assert _refused(L, one(**kw)), kw
            assert (host_dst == SENT).all(), kw
        assert one(r=E.h) == 0 and (host_dst == SENT).all()
        assert one() == 0 and (host_dst[:32] == 9).all() and (host_dst[32:] == SENT).all()

        kps = np.full(8, 7, orbgpu_mod.KP_DTYPE)
        desc = np.full((8, 32), 7, np.uint8)
        n = ctypes.c_int(7)

        def ext(r=A.h, s=host_src.ctypes.data, sw=8, sh=4, ss=8, pn=ctypes.byref(n)):
            return L.orb_extract_rectified(ctx.h, r, s, sw, sh, ss, kps.ctypes.data, 8, pn, desc.ctypes.data)

        for kw in (dict(r=None), dict(sw=-1), dict(sh=-1), dict(ss=7), dict(sw=4097, ss=4097), dict(sh=4097),
                   dict(pn=None)):
            assert _refused(L, ext(**kw)), kw
            assert n.value == 7 and (desc == 7).all() and kps.tobytes() == np.full(8, 7, orbgpu_mod.KP_DTYPE).tobytes()
        # empty images: ORB_OK, outputs untouched
        assert ext(s=None) == 0 and ext(sw=0) == 0 and ext(r=E.h) == 0
        assert n.value == 7 and (desc == 7).all()
    finally:
        for r in (A, B, E):
            r.close()
        src.close()
        dst.close()
