"""k_front_prep and k_bird_mask on the GPU, byte for byte against the CPU definitions orb_front_prep_host and
orb_bird_mask_host (themselves checked against the numpy restatement in test_prep_host.py): the widths, alignments and
strides at which the kernels take their byte paths, the batch forms, the chain into orb_extract_batch_device on one
stream, the host-frame form orb_extract_fisheye with the driver's own geometry, the birdview chain and the C++ mirror."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import prep_ref as ref
from conftest import GOLDEN, PKG, ROOT

pytestmark = pytest.mark.gpu
SENT = 0xA5
ARG = -1
CODES = (ref.GRAY, ref.RGB, ref.BGR, ref.RGBA, ref.BGRA)
CPP = os.path.join(ROOT, "tests", "cpp_prep")
# a 150 x 100 image holds three pyramid levels of the extractor: a level needs 62 pixels a side (one 30-pixel cell
# between the borders), and level 3 of 100 rows has 58
LEVELS = 3


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


def _color(code):
    return None if code == ref.GRAY else code


def _image(rng, n, h, w, code):
    c = ref.channels(code)
    return rng.integers(0, 256, (n, h, w) if c == 1 else (n, h, w, c), dtype=np.uint8)


def _mask(rng, h, w, mc):
    if mc == 0:
        return None
    vals = np.array([0, 249, 250, 251, 252, 255], np.uint8)
    return np.ascontiguousarray(vals[rng.integers(0, len(vals), (h, w) if mc == 1 else (h, w, 3))])


def _lay(rows, base, stride, pitch, total, fill):
    """rows (n, h, bytes) at base + f * pitch + y * stride of a buffer of `total` bytes filled with `fill`."""
    buf = np.full(total, fill, np.uint8)
    n, h, b = rows.shape
    for f in range(n):
        for y in range(h):
            o = base + f * pitch + y * stride
            buf[o:o + b] = rows[f, y]
    return buf


def _prep_batch(orbgpu, L, ctx, src, dst, prep, code, imgs, want, so=0, do=0, spad=0, dpad=0, sgap=0, dgap=0):
    """imgs (n, sh, sw[, C]) at src.p + so with row stride sw * C + spad and frame pitch sh * stride + sgap, prepared
    into dst.p + do likewise: the whole destination buffer must equal `want` (n, oh, ow) inside the rows and the
    sentinel everywhere else."""
    n, sh = imgs.shape[:2]
    rows = imgs.reshape(n, sh, -1)
    _, oh, ow = want.shape
    srs, drs = rows.shape[2] + spad, ow + dpad
    sfp, dfp = sh * srs + sgap, oh * drs + dgap
    s = _lay(rows, so, srs, sfp, so + n * sfp + 8, 0xEE)
    exp = _lay(want, do, drs, dfp, do + n * dfp + 16, SENT)
    src.put(s)
    dst.put(np.full(len(exp), SENT, np.uint8))
    orbgpu.front_prep_device(ctx, prep, _color(code), src.p + so, n, sfp, srs, dst.p + do, dfp, drs)
    assert L.orb_sync(ctx.h) == 0
    return np.array_equal(dst.get(len(exp)), exp)


def _want(orbgpu, imgs, mask, crop, code):
    out = np.stack([orbgpu.front_prep_host(im, mask, crop, _color(code)) for im in imgs])
    assert np.array_equal(out[0], ref.front_prep(imgs[0], mask, crop, code))
    return out


def test_widths_alignments_strides(orbgpu_mod, L, ctx):
    """Every code; output widths 1, 2, 3, 4, 5, 7, 8, 9, 65 and 257 (quads inside a row, the partial last quad, more
    than one block); output heights 1, 2, 5; cx in 0..3 (cx * C mod 4 over all four values for C = 1 and 3); source and
    destination bases offset by 0..3 bytes; row strides that are odd and that are multiples of 4; 1, 2 and 3 frames with
    frame pitches that are no multiples of 4; no, 1- and 3-channel masks.  The destination equals the host definition's
    and every byte of its padding, before its base and past its end keeps the sentinel."""
    src, dst = Dev(L, ctx, 1 << 17), Dev(L, ctx, 1 << 14)
    rng = np.random.default_rng(31)
    mods, k = set(), 0
    try:
        for code in CODES:
            C = ref.channels(code)
            for ow in (1, 2, 3, 4, 5, 7, 8, 9, 65, 257):
                if ow == 257 and code != ref.BGR:
                    continue
                for cx in range(4):
                    k += 1
                    oh, n = (1, 2, 5)[k % 3], (1, 2, 3)[(k // 3) % 3]
                    cy = k % 3
                    sw, sh = cx + 2 * ow + k % 2, cy + 2 * oh + (k // 2) % 2
                    crop = (cx, cy, 2 * ow, 2 * oh)
                    imgs = _image(rng, n, sh, sw, code)
                    mask = _mask(rng, sh, sw, (0, 1, 3)[k % 3])
                    want = _want(orbgpu_mod, imgs, mask, crop, code)
                    prep = orbgpu_mod.FrontPrep(ctx, (sw, sh), mask, crop)
                    try:
                        assert prep.size == (ow, oh) and prep.source_size == (sw, sh)
                        # the row base is src + so + y * stride: aligned bases and strides take the wide path when
                        # cx * C is a multiple of 4, every other combination the byte path
                        spad = (-(sw * C)) % 4 if k % 2 else (1, 3, 2)[k % 3]
                        dpad = (-ow) % 4 if k % 4 < 2 else (1, 3)[k % 2]
                        so, do = (k // 2) % 4 if k % 5 else 0, (k // 3) % 4 if k % 7 else 0
                        assert _prep_batch(orbgpu_mod, L, ctx, src, dst, prep, code, imgs, want, so, do, spad, dpad,
                                           sgap=(1, 2, 3, 5)[k % 4], dgap=(3, 1, 6)[k % 3]), (code, ow, oh, cx, n, so, do)
                        mods.add((C, (cx * C) % 4))
                    finally:
                        prep.close()
        for C in (1, 3):
            assert {m for c, m in mods if c == C} == {0, 1, 2, 3}
        # one width, every base offset on both sides, with aligned strides: the wide path and the byte path in turn
        for code in (ref.GRAY, ref.BGR, ref.RGBA):
            C = ref.channels(code)
            sw, sh, crop = 40, 6, (4, 1, 36, 4)
            imgs = _image(rng, 2, sh, sw, code)
            mask = _mask(rng, sh, sw, 3)
            want = _want(orbgpu_mod, imgs, mask, crop, code)
            prep = orbgpu_mod.FrontPrep(ctx, (sw, sh), mask, crop)
            try:
                for so in range(4):
                    for do in range(4):
                        assert _prep_batch(orbgpu_mod, L, ctx, src, dst, prep, code, imgs, want, so, do, 0, 2, 0, 0), \
                            (code, so, do)
            finally:
                prep.close()
    finally:
        src.close()
        dst.close()


def test_no_mask_and_full_masks(orbgpu_mod, L, ctx):
    """No mask keeps everything; an all-masked camera gives zeros; the mean counts a masked pixel as 0 on the GPU too."""
    src, dst = Dev(L, ctx, 1 << 14), Dev(L, ctx, 1 << 12)
    try:
        imgs = np.full((1, 4, 16, 3), 200, np.uint8)
        for mask, val in ((None, 200), (np.full((4, 16), 251, np.uint8), 0), (np.full((4, 16), 250, np.uint8), 200)):
            prep = orbgpu_mod.FrontPrep(ctx, (16, 4), mask, (0, 0, 16, 4))
            try:
                assert _prep_batch(orbgpu_mod, L, ctx, src, dst, prep, ref.BGR, imgs, np.full((1, 2, 8), val, np.uint8))
            finally:
                prep.close()
        mask = np.zeros((4, 16), np.uint8)
        mask[0, ::2] = 255   # S00 of every block of the first output row
        prep = orbgpu_mod.FrontPrep(ctx, (16, 4), mask, (0, 0, 16, 4))
        try:
            want = np.array([[[150] * 8, [200] * 8]], np.uint8)
            assert _prep_batch(orbgpu_mod, L, ctx, src, dst, prep, ref.BGR, imgs, want)
        finally:
            prep.close()
    finally:
        src.close()
        dst.close()


def _bird_batch(orbgpu, L, ctx, src, dst, masks, want, so, do, spad, dpad, sgap, dgap):
    n, h, w, c = masks.shape
    srs, drs = w * c + spad, w + dpad
    sfp, dfp = h * srs + sgap, h * drs + dgap
    s = _lay(masks.reshape(n, h, -1), so, srs, sfp, so + n * sfp + 8, 0xEE)
    exp = _lay(want, do, drs, dfp, do + n * dfp + 16, SENT)
    src.put(s)
    dst.put(np.full(len(exp), SENT, np.uint8))
    orbgpu.bird_mask_device(ctx, c, src.p + so, n, w, h, sfp, srs, dst.p + do, dfp, drs)
    assert L.orb_sync(ctx.h) == 0
    return np.array_equal(dst.get(len(exp)), exp)


@pytest.mark.parametrize("w,h", [(160, 200), (64, 64), (37, 53)])
def test_bird_mask_device(orbgpu_mod, L, ctx, w, h):
    """orb_bird_mask_device equals orb_bird_mask_host: the footprint inside, clipped, and at an odd size; 3 and 4
    channels; one frame and three frames with differing masks; offset bases, odd strides and frame pitches."""
    src, dst = Dev(L, ctx, 1 << 19), Dev(L, ctx, 1 << 17)
    rng = np.random.default_rng(w)
    try:
        for c in (3, 4):
            for n in (1, 3):
                masks = rng.integers(0, 40, (n, h, w, c), dtype=np.uint8)
                want = np.stack([orbgpu_mod.bird_mask_host(m) for m in masks])
                assert np.array_equal(want[0], ref.bird_mask(masks[0]))
                if (w, h) == (37, 53):     # the footprint (58 x 98 around the centre) covers the whole mask
                    assert not want.any()
                else:
                    assert (want == 250).any() and (want == 0).any()
                    assert n == 1 or not np.array_equal(want[0], want[1])
                assert _bird_batch(orbgpu_mod, L, ctx, src, dst, masks, want, 0, 0, (-(w * c)) % 4, (-w) % 4, 0, 0)
                assert _bird_batch(orbgpu_mod, L, ctx, src, dst, masks, want, 1, 2, 3, 1, 5, 7)
                assert _bird_batch(orbgpu_mod, L, ctx, src, dst, masks, want, 3, 1, 0, 0, 2, 1)
    finally:
        src.close()
        dst.close()


def test_chain_into_batch_extraction(orbgpu_mod):
    """front_prep_device into orb_extract_batch_device on one stream with no synchronisation between: 320 x 240 BGR
    frames cropped to 300 x 200 give 150 x 100 frames; the results equal the batch extraction of the host-prepared
    frames."""
    from orbgpu.synth import synth_frame
    n, sw, sh, crop = 3, 320, 240, (10, 20, 300, 200)
    gray = np.stack([synth_frame(sw, sh, 40 + f) for f in range(n)])
    rng = np.random.default_rng(8)
    # a colour frame whose channels differ, so that the weights matter
    frames = np.stack([gray, np.roll(gray, 3, axis=2), 255 - gray], axis=-1)
    mask = np.zeros((sh, sw, 3), np.uint8)
    mask[:, :, 1] = np.where(rng.random((sh, sw)) < 0.02, 255, 0)
    mask[:60, :80, 1] = 255
    want = np.stack([orbgpu_mod.front_prep_host(f, mask, crop, orbgpu_mod.COLOR_BGR) for f in frames])
    assert want.shape == (n, 100, 150) and not want[:, :20, :35].any()
    a = orbgpu_mod.BatchExtractor(500, 150, 100, n, nlevels=LEVELS)
    b = orbgpu_mod.BatchExtractor(500, 150, 100, n, nlevels=LEVELS)
    prep = orbgpu_mod.FrontPrep(a, (sw, sh), mask, crop)
    try:
        a.upload_fisheye(frames, prep, orbgpu_mod.COLOR_BGR)
        a.launch()          # (same stream: no sync in between)
        a.sync()
        b.upload(want)
        b.launch()
        b.sync()
        assert np.array_equal(a.counts(), b.counts()) and (a.counts() > 30).all()
        for f in range(n):
            (ka, da), (kb, db) = a.results(f), b.results(f)
            assert ka.tobytes() == kb.tobytes() and np.array_equal(da, db)
            assert np.array_equal(a.debug_level_image(0, f), want[f])
    finally:
        prep.close()
        a.close()
        b.close()


@pytest.mark.parametrize("code", [ref.GRAY, ref.BGR])
def test_extract_fisheye_equals_extract_of_host_image(orbgpu_mod, code):
    from orbgpu.synth import synth_frame
    sw, sh, crop = 330, 250, (7, 9, 300, 200)
    gray = synth_frame(sw, sh, 12)
    frame = gray if code == ref.GRAY else np.stack([gray, np.roll(gray, 2, axis=1), np.roll(gray, 5, axis=0)], axis=-1)
    mask = np.zeros((sh, sw), np.uint8)
    mask[100:140, 150:230] = 255
    img = orbgpu_mod.front_prep_host(frame, mask, crop, _color(code))
    assert np.array_equal(img, ref.front_prep(frame, mask, crop, code))
    e, p = orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7), orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7)
    prep = orbgpu_mod.FrontPrep(e, (sw, sh), mask, crop)
    try:
        k, d = e(frame, color=_color(code), prep=prep)
        lvl0 = e.mvImagePyramid[0]
        qk, qd = p(img)
        assert len(k) > 50 and k.tobytes() == qk.tobytes() and np.array_equal(d, qd)
        assert np.array_equal(lvl0, img)
        # rows with padding go down as they are
        wide = np.zeros((sh, sw + 5) + frame.shape[2:], np.uint8)
        wide[:, :sw] = frame
        k2, d2 = e(wide[:, :sw], color=_color(code), prep=prep)
        assert k2.tobytes() == qk.tobytes() and np.array_equal(d2, qd)
        # an empty image leaves the outputs as given
        assert e(np.zeros((0, 0), np.uint8), keypoints="k", descriptors="d", prep=prep) == ("k", "d")
    finally:
        prep.close()
        e.close()
        p.close()


def test_driver_geometry_equals_fixture(orbgpu_mod):
    """The driver's own geometry: orb_extract_fisheye over synth_frame(1920, 1208, 0) with the reference's camera mask,
    crop (0, 0, 1900, 800) and fisheye.yaml's extractor (2000, 1.2, 8, 15, 5) gives the fixture's keypoints."""
    from orbgpu.synth import synth_frame
    g = np.load(os.path.join(GOLDEN, "mask_new_front.npz"))
    keep = np.unpackbits(g["keep_bits"], axis=1)[:, :int(g["shape"][1])].astype(bool)
    mask = np.where(keep, 0, 255).astype(np.uint8)
    e = orbgpu_mod.ORBextractor(2000, 1.2, 8, 15, 5)
    prep = orbgpu_mod.FrontPrep(e, (1920, 1208), mask, (0, 0, 1900, 800))
    try:
        assert prep.size == (950, 400)
        k, d = e(synth_frame(1920, 1208, 0), prep=prep)
        assert len(k) == len(g["kps_0"]) > 1900
        assert k.tobytes() == g["kps_0"].tobytes() and np.array_equal(d, g["desc_0"])
    finally:
        prep.close()
        e.close()


def test_birdview_chain(orbgpu_mod, L, ctx):
    """A mask converted on the device goes to orb_bird_extract_device after orb_sync: the extraction equals the one
    with the host-converted mask."""
    from orbgpu.synth import synth_bird_mask, synth_frame
    w, h = 320, 240
    img = synth_frame(w, h, 3)
    valid = synth_bird_mask(w, h, 1)
    m3 = np.zeros((h, w, 3), np.uint8)
    m3[:, :, 1] = np.where(valid > 0, 200, 7)
    m3[:, :, 0] = 255
    host_mask = orbgpu_mod.bird_mask_host(m3)
    assert set(np.unique(host_mask)) == {0, 250}
    bird = orbgpu_mod.BirdORB(500)
    d_img, d_src, d_mask = Dev(L, ctx, w * h), Dev(L, ctx, w * h * 3), Dev(L, ctx, w * h)
    try:
        d_img.put(img)
        d_src.put(m3)
        orbgpu_mod.bird_mask_device(ctx, 3, d_src.p, 1, w, h, 0, w * 3, d_mask.p, 0, w)
        assert L.orb_sync(ctx.h) == 0          # (the birdview object has a stream of its own)
        assert np.array_equal(d_mask.get().reshape(h, w), host_mask)
        k, d = bird.extract_device(d_img.p, w, h, d_mask.p)
        qk, qd = bird.extract(img, host_mask)
        assert len(k) > 50 and k.tobytes() == qk.tobytes() and np.array_equal(d, qd)
    finally:
        for x in (d_img, d_src, d_mask):
            x.close()
        bird.close()


def _refused(L, st):
    msg = L.orb_last_error() or b""
    return st == ARG and b"NULL context" not in msg


def test_argument_errors_with_handles(orbgpu_mod, L, ctx):
    """Every refusal of the handle-taking calls: ORB_ERR_ARG before any GPU work, the destination and outputs untouched."""
    mask = np.zeros((8, 12), np.uint8)
    out = ctypes.c_void_p()

    def create(sw=12, sh=8, m=mask, mc=1, ms=12, cx=0, cy=0, cw=8, ch=4, o=ctypes.byref(out)):
        return L.orb_prep_create(ctx.h, sw, sh, None if m is None else m.ctypes.data, mc, ms, cx, cy, cw, ch, o)

    for kw in (dict(o=None), dict(mc=2), dict(mc=4), dict(cw=7), dict(ch=3), dict(cw=-2), dict(cx=-1), dict(cy=-1),
               dict(cx=5), dict(cy=5), dict(sw=8193, ms=8193), dict(sh=8193), dict(sw=-1), dict(ms=11)):
        assert _refused(L, create(**kw)) and not out, kw
    A = orbgpu_mod.FrontPrep(ctx, (12, 8), mask, (0, 0, 8, 4))
    E = orbgpu_mod.FrontPrep(ctx, (12, 8), None, (2, 2, 0, 4))
    src, dst = Dev(L, ctx, 4096), Dev(L, ctx, 4096)
    try:
        assert E.size == (0, 2) and A.size == (4, 2)
        src.put(np.full(4096, 9, np.uint8))
        dst.put(np.full(4096, SENT, np.uint8))

        def dev(p=A.h, code=ref.BGR, s=src.p, n=2, sfp=288, srs=36, d=dst.p, dfp=8, drs=4):
            return L.orb_front_prep_device(ctx.h, p, code, s, n, sfp, srs, d, dfp, drs)

        for kw in (dict(p=None), dict(code=4), dict(code=-2), dict(s=None), dict(d=None), dict(n=-1), dict(srs=35),
                   dict(drs=3), dict(sfp=287), dict(dfp=7), dict(code=ref.BGRA), dict(code=ref.GRAY, srs=11)):
            assert _refused(L, dev(**kw)), kw
        assert dev(n=0, s=None, d=None) == 0 and dev(p=E.h, s=None, d=None) == 0
        assert L.orb_sync(ctx.h) == 0 and (dst.get() == SENT).all()
        assert dev(n=1, sfp=0, dfp=0) == 0 and L.orb_sync(ctx.h) == 0       # one frame: the pitches are not read
        got = dst.get()
        assert (got[:8] == 9).all() and (got[8:] == SENT).all()

        host = np.full(8 * 36, 9, np.uint8)
        kps = np.full(8, 7, orbgpu_mod.KP_DTYPE)
        desc = np.full((8, 32), 7, np.uint8)
        n = ctypes.c_int(7)

        def ext(p=A.h, code=ref.BGR, s=host.ctypes.data, ss=36, pn=ctypes.byref(n)):
            return L.orb_extract_fisheye(ctx.h, p, code, s, ss, kps.ctypes.data, 8, pn, desc.ctypes.data)

        for kw in (dict(p=None), dict(code=5), dict(ss=35), dict(pn=None)):
            assert _refused(L, ext(**kw)), kw
            assert n.value == 7 and (desc == 7).all() and kps.tobytes() == np.full(8, 7, orbgpu_mod.KP_DTYPE).tobytes()
        assert ext(s=None) == 0 and ext(p=E.h) == 0 and n.value == 7 and (desc == 7).all()

        def bm(c=3, s=src.p, nf=2, w=6, h=4, sfp=72, srs=18, d=dst.p, dfp=24, drs=6):
            return L.orb_bird_mask_device(ctx.h, c, s, nf, w, h, sfp, srs, d, dfp, drs)

        dst.put(np.full(4096, SENT, np.uint8))
        for kw in (dict(c=1), dict(c=5), dict(s=None), dict(d=None), dict(nf=-1), dict(w=-1), dict(h=-1),
                   dict(w=4097, srs=3 * 4097, drs=4097, sfp=1 << 20, dfp=1 << 20), dict(h=4097, sfp=1 << 20, dfp=1 << 20),
                   dict(srs=17), dict(drs=5), dict(sfp=71), dict(dfp=23)):
            assert _refused(L, bm(**kw)), kw
        assert bm(nf=0, s=None, d=None) == 0 and bm(w=0) == 0 and bm(h=0) == 0
        assert L.orb_sync(ctx.h) == 0 and (dst.get() == SENT).all()
    finally:
        A.close()
        E.close()
        src.close()
        dst.close()


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_prep_mirror")


def test_cpp_mirror(orbgpu_mod, mirror_bin, tmp_path):
    """The C++ FrontPrep: operator() on a raw gray and a raw BGR frame, mvImagePyramid[0] and ConvertMaskBirdview,
    against the host definitions and the extraction of the host-prepared image."""
    from orbgpu.synth import synth_frame
    sw, sh, crop, code = 330, 250, (7, 9, 300, 200), ref.BGR
    gray = synth_frame(sw, sh, 21)
    colour = np.ascontiguousarray(np.stack([gray, np.roll(gray, 2, axis=1), np.roll(gray, 5, axis=0)], axis=-1))
    mask = np.zeros((sh, sw, 3), np.uint8)
    mask[60:120, 100:200, 1] = 255
    rng = np.random.default_rng(4)
    bird = rng.integers(0, 40, (53, 37, 3), dtype=np.uint8)
    src, dst = tmp_path / "case.bin", tmp_path / "results.bin"
    with open(src, "wb") as fh:
        fh.write(np.array([sw, sh, *crop, 3, code, LEVELS, 37, 53], np.int32).tobytes())
        for a in (mask, gray, colour, bird):
            fh.write(np.ascontiguousarray(a).tobytes())
    p = subprocess.run([mirror_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    buf = dst.read_bytes()
    assert np.frombuffer(buf, np.int32, 2).tolist() == [150, 100]
    pos = 8
    e = orbgpu_mod.ORBextractor(500, 1.2, LEVELS, 20, 7)
    try:
        for frame, c in ((gray, ref.GRAY), (colour, code)):
            img = orbgpu_mod.front_prep_host(frame, mask, crop, _color(c))
            qk, qd = e(img)
            n = int(np.frombuffer(buf, np.int32, 1, pos)[0])
            pos += 4
            assert n == len(qk) > 50
            assert buf[pos:pos + 28 * n] == qk.tobytes()
            pos += 28 * n
            assert buf[pos:pos + 32 * n] == qd.tobytes()
            pos += 32 * n
            assert buf[pos:pos + img.size] == img.tobytes()
            pos += img.size
        assert buf[pos:] == orbgpu_mod.bird_mask_host(bird).tobytes()
    finally:
        e.close()
