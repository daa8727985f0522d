"""k_to_gray on the GPU, byte for byte against the integer formula in numpy (rgbd_ref.py): the whole RGB cube, the
shapes, alignments and strides at which the kernel takes its byte path, and the chains orb_to_gray_device feeds
(orb_extract_batch_device, orb_extract_color, orb_bird_extract_device)."""
import ctypes

import numpy as np
import pytest

import rgbd_ref as ref

pytestmark = pytest.mark.gpu
SENT = 0xA5


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


def _sync(L, ctx):
    assert L.orb_sync(ctx.h) == 0


def test_whole_rgb_cube(L, ctx):
    """One 4096 x 4096 RGB frame holding every (R, G, B) once, one launch."""
    idx = np.arange(1 << 24, dtype=np.uint32)
    cube = np.empty((1 << 24, 3), np.uint8)
    cube[:, 0], cube[:, 1], cube[:, 2] = idx >> 16, (idx >> 8) & 255, idx & 255
    want = ref.gray_rgb(cube[:, 0], cube[:, 1], cube[:, 2])
    src, dst = Dev(L, ctx, cube.nbytes), Dev(L, ctx, 1 << 24)
    try:
        src.put(cube)
        assert L.orb_to_gray_device(ctx.h, ref.COLOR_RGB, src.p, 1, 4096, 4096, 0, 3 * 4096, dst.p, 0, 4096) == 0
        _sync(L, ctx)
        assert np.array_equal(dst.get(), want)
    finally:
        src.close()
        dst.close()


@pytest.mark.parametrize("code", [ref.COLOR_RGB, ref.COLOR_BGR, ref.COLOR_RGBA, ref.COLOR_BGRA])
def test_shapes_alignments_strides(L, ctx, code):
    """w in {1, 3, 4, 5, 63, 64, 65, 257} x h = 3, bases offset by 0..3 bytes on either side, row strides w c, w c + 1,
    w c + 7, frame pitches that are no multiple of 4, 1 / 2 / 5 frames: the destination equals numpy's, and every byte
    of its padding, before its base and past the last frame keeps the sentinel."""
    ch = ref.CHANNELS[code]
    h = 3
    rng = np.random.default_rng(100 + code)
    src, dst = Dev(L, ctx, 1 << 16), Dev(L, ctx, 1 << 14)
    odd_pitch = 0
    try:
        for w in (1, 3, 4, 5, 63, 64, 65, 257):
            for pad in (0, 1, 7):
                for nf in (1, 2, 5):
                    srs, drs = w * ch + pad, w + pad
                    sfp, dfp = h * srs + 3, h * drs + 1
                    odd_pitch += (sfp % 4 != 0) + (dfp % 4 != 0)
                    img = rng.integers(0, 256, (nf, h, w, ch), dtype=np.uint8)
                    gray = ref.to_gray(img, code)
                    sbuf = rng.integers(0, 256, nf * sfp + 8, dtype=np.uint8)
                    for so in range(4):
                        for do in range(4):
                            s = sbuf.copy()
                            exp = np.full(nf * dfp + 16, SENT, np.uint8)
                            for f in range(nf):
                                for y in range(h):
                                    o = so + f * sfp + y * srs
                                    s[o:o + w * ch] = img[f, y].ravel()
                                    o = do + f * dfp + y * drs
                                    exp[o:o + w] = gray[f, y]
                            src.put(s)
                            dst.put(np.full(len(exp), SENT, np.uint8))
                            st = L.orb_to_gray_device(ctx.h, code, src.p + so, nf, w, h, sfp, srs, dst.p + do, dfp, drs)
                            assert st == 0
                            _sync(L, ctx)
                            got = dst.get(len(exp))
                            assert np.array_equal(got, exp), (w, pad, nf, so, do)
        assert odd_pitch > 100
    finally:
        src.close()
        dst.close()


def _color_frames(orbgpu, w, h, n, first=0):
    """n BGR frames with texture in every channel (three synthetic scenes each)."""
    from orbgpu.synth import synth_frame
    return np.stack([np.stack([synth_frame(w, h, first + 3 * f + c) for c in range(3)], -1) for f in range(n)])


def test_chain_into_batch_extraction(orbgpu_mod):
    w, h = 320, 240
    bgr = _color_frames(orbgpu_mod, w, h, 2)
    gray = ref.to_gray(bgr, ref.COLOR_BGR)
    ext = orbgpu_mod.BatchExtractor(500, w, h, 2)
    try:
        ext.upload_color(bgr, orbgpu_mod.COLOR_BGR)
        ext.launch()
        ext.sync()
        got = [tuple(a.copy() for a in ext.results(f)) for f in range(2)]
        ext.upload(gray)
        ext.launch()
        ext.sync()
        for f in range(2):
            k, d = ext.results(f)
            assert len(k) > 100
            assert got[f][0].tobytes() == k.tobytes() and np.array_equal(got[f][1], d), f
    finally:
        ext.close()


@pytest.mark.parametrize("code", [ref.COLOR_BGR, ref.COLOR_RGBA])
def test_extract_color_equals_extract_of_the_gray(orbgpu_mod, code):
    w, h = 321, 243   # (rows whose colour stride is no multiple of 4 on the host side)
    bgr = _color_frames(orbgpu_mod, w, h, 1, first=7)[0]
    img = bgr if code == ref.COLOR_BGR else np.concatenate([bgr[..., ::-1], np.full((h, w, 1), 77, np.uint8)], -1)
    gray = ref.to_gray(img, code)
    ext = orbgpu_mod.ORBextractor(500, 1.2, 8, 20, 7)
    try:
        k1, d1 = ext(img, color=code)
        lvl0 = ext.mvImagePyramid[0]
        k2, d2 = ext(gray)
        assert len(k1) > 100 and k1.tobytes() == k2.tobytes() and np.array_equal(d1, d2)
        assert np.array_equal(lvl0, gray)
        # an empty image leaves the outputs as given
        assert ext(np.zeros((0, 0, 3), np.uint8), keypoints="k", descriptors="d", color=ref.COLOR_BGR) == ("k", "d")
    finally:
        ext.close()


def test_bird_extract_on_a_device_converted_frame(orbgpu_mod, L, ctx):
    w, h = 320, 240
    bgr = _color_frames(orbgpu_mod, w, h, 1, first=11)[0]
    gray = ref.to_gray(bgr, ref.COLOR_BGR)
    bird = orbgpu_mod.BirdORB(500)
    d_col, d_gray, d_host = Dev(L, ctx, bgr.nbytes), Dev(L, ctx, w * h), Dev(L, ctx, w * h)
    try:
        d_col.put(bgr)
        d_host.put(gray)
        assert L.orb_to_gray_device(ctx.h, ref.COLOR_BGR, d_col.p, 1, w, h, 0, 3 * w, d_gray.p, 0, w) == 0
        _sync(L, ctx)   # the birdview object has a stream of its own
        k1, d1 = bird.extract_device(d_gray.p, w, h)
        k2, d2 = bird.extract_device(d_host.p, w, h)
        assert len(k1) > 50 and k1.tobytes() == k2.tobytes() and np.array_equal(d1, d2)
    finally:
        for d in (d_col, d_gray, d_host):
            d.close()
        bird.close()
