"""The fisheye driver's input path on the CPU: orb_front_prep_host (applyMask, crop, half-size resize, cvtColor) and
orb_bird_mask_host (ConvertMaskBirdview) against the independent numpy restatement tests/prep_ref.py, the decisions of
the definition planted one by one in tiny images with the answer written by hand, the repository's fisheye fixture, every
argument error, and the definitions of csrc/prep_def.h under ASan + UBSan in a stand-alone program.  No GPU."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import prep_ref as ref
from conftest import GOLDEN, ROOT

ARG = -1
SENT = 0xA5
CODES = (ref.GRAY, ref.RGB, ref.BGR, ref.RGBA, ref.BGRA)


@pytest.fixture(scope="module")
def L(orbgpu_mod):
    from orbgpu import _lib
    return _lib.lib()


def _ptr(a, off=0):
    return ctypes.c_void_p(a.ctypes.data + off) if a is not None else None


def _laid(img, off, pad, fill=0xEE):
    """img (h, w[, c]) as bytes at `off` of a buffer with row stride w * c + pad; returns (buffer, stride)."""
    h = img.shape[0]
    row = img.reshape(h, -1)
    stride = row.shape[1] + pad
    buf = np.full(off + h * stride + 8, fill, np.uint8)
    for y in range(h):
        buf[off + y * stride:off + y * stride + row.shape[1]] = row[y]
    return buf, stride


def prep_host(L, code, img, mask, crop, so=0, spad=0, mo=0, mpad=0, do=0, dpad=0):
    """orb_front_prep_host through the C ABI with offset bases and padded strides; the destination's padding must keep
    its sentinel.  Returns the (ch / 2, cw / 2) image."""
    sh, sw = img.shape[:2]
    cx, cy, cw, ch = crop
    s, srs = _laid(img, so, spad)
    m, mrs, mc = None, 0, 1
    if mask is not None:
        m, mrs = _laid(mask, mo, mpad)
        mc = 1 if mask.ndim == 2 else 3
    ow, oh = cw // 2, ch // 2
    drs = ow + dpad
    d = np.full(do + oh * drs + 8, SENT, np.uint8)
    st = L.orb_front_prep_host(code, _ptr(s, so), sw, sh, srs, _ptr(m, mo), mc, mrs, cx, cy, cw, ch, _ptr(d, do), drs)
    assert st == 0, st
    out = np.zeros((oh, ow), np.uint8)
    keep = np.ones(len(d), bool)
    for y in range(oh):
        out[y] = d[do + y * drs:do + y * drs + ow]
        keep[do + y * drs:do + y * drs + ow] = False
    assert (d[keep] == SENT).all(), "a byte outside [row, row + cw / 2) was written"
    return out


def _image(rng, h, w, code):
    c = ref.channels(code)
    return rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)


def _mask(rng, h, w, mc):
    """Mask bytes around the threshold: 249..252 and the extremes, so both sides of > 250 are dense."""
    if mc == 0:
        return None
    vals = np.array([0, 249, 250, 251, 252, 255], np.uint8)
    m = vals[rng.integers(0, len(vals), (h, w) if mc == 1 else (h, w, 3))]
    return np.ascontiguousarray(m)


def test_front_prep_matches_reference(L):
    """Random sources from 2 x 2 to 70 x 40: every code, no / 1- / 3-channel masks, cx * C mod 4 over all four values,
    odd strides and base offsets 1..3 on the source, the mask and the destination."""
    rng = np.random.default_rng(2024)
    seen_mod, n = set(), 0
    for code in CODES:
        C = ref.channels(code)
        for k in range(24):
            sw, sh = int(rng.integers(2, 71)), int(rng.integers(2, 41))
            if k == 0:
                sw, sh = 2, 2
            cw = 2 * int(rng.integers(1, sw // 2 + 1))
            ch = 2 * int(rng.integers(1, sh // 2 + 1))
            cx = min(k % 4, sw - cw) if k < 8 else int(rng.integers(0, sw - cw + 1))
            cy = int(rng.integers(0, sh - ch + 1))
            img = _image(rng, sh, sw, code)
            mask = _mask(rng, sh, sw, k % 3 if k % 3 < 2 else 3)
            want = ref.front_prep(img, mask, (cx, cy, cw, ch), code)
            got = prep_host(L, code, img, mask, (cx, cy, cw, ch), so=k % 4, spad=(1, 0, 3, 7)[k % 4], mo=(k + 1) % 4,
                            mpad=k % 3, do=(k + 2) % 4, dpad=(0, 1, 5)[k % 3])
            assert np.array_equal(got, want), (code, k, sw, sh, cx, cy, cw, ch)
            seen_mod.add((C, (cx * C) % 4))
            n += 1
    for C in (1, 3):
        assert {m for c, m in seen_mod if c == C} == {0, 1, 2, 3}
    assert n == 120


def test_python_mirror_matches_reference(orbgpu_mod):
    rng = np.random.default_rng(5)
    for code in CODES:
        img = _image(rng, 20, 34, code)
        for mask in (None, _mask(rng, 20, 34, 1), _mask(rng, 20, 34, 3)):
            got = orbgpu_mod.front_prep_host(img, mask, (3, 2, 30, 16), None if code == ref.GRAY else code)
            assert np.array_equal(got, ref.front_prep(img, mask, (3, 2, 30, 16), code))
    m = rng.integers(0, 40, (53, 37, 3), dtype=np.uint8)
    assert np.array_equal(orbgpu_mod.bird_mask_host(m), ref.bird_mask(m))


# ---- planted decisions: tiny images, the answers written by hand ----

def test_planted_rounding(L):
    """Block sums congruent to 0, 1, 2, 3 mod 4: (s + 2) >> 2, so a sum of 4 k + 2 rounds up and 4 k + 1 down."""
    img = np.array([[4, 4, 4, 4, 4, 4, 4, 4],
                    [4, 4, 4, 5, 4, 6, 4, 7]], np.uint8)   # sums 16, 17, 18, 19
    assert prep_host(L, ref.GRAY, img, None, (0, 0, 8, 2)).tolist() == [[4, 4, 5, 5]]
    img = np.array([[255, 255], [255, 255]], np.uint8)
    assert prep_host(L, ref.GRAY, img, None, (0, 0, 2, 2)).tolist() == [[255]]
    img = np.array([[0, 1], [0, 0]], np.uint8)       # 1 -> 0
    assert prep_host(L, ref.GRAY, img, None, (0, 0, 2, 2)).tolist() == [[0]]
    img = np.array([[1, 1], [0, 0]], np.uint8)       # 2 -> 1
    assert prep_host(L, ref.GRAY, img, None, (0, 0, 2, 2)).tolist() == [[1]]


def test_planted_mask_threshold_and_mean(L):
    """Mask byte 250 keeps, 251 zeroes; the zeroed pixel stays in the mean as a 0 (it is not left out of it)."""
    img = np.full((2, 4), 100, np.uint8)
    mask = np.array([[250, 0, 251, 0], [0, 0, 0, 0]], np.uint8)
    # block 0: nothing masked -> 100; block 1: one pixel zeroed -> (300 + 2) >> 2 = 75, not 100
    assert prep_host(L, ref.GRAY, img, mask, (0, 0, 4, 2)).tolist() == [[100, 75]]
    # a 3-channel mask is read at channel 1 only
    m3 = np.zeros((2, 4, 3), np.uint8)
    m3[0, 0] = (255, 250, 255)
    m3[0, 2] = (0, 251, 0)
    assert prep_host(L, ref.GRAY, img, m3, (0, 0, 4, 2)).tolist() == [[100, 75]]
    # every channel of a masked colour pixel is zeroed
    c = np.full((2, 2, 3), 200, np.uint8)
    mk = np.array([[255, 0], [0, 0]], np.uint8)
    assert prep_host(L, ref.BGR, c, mk, (0, 0, 2, 2)).tolist() == [[150]]   # each channel (600 + 2) >> 2 = 150


def test_planted_mask_in_source_coordinates(L):
    """The mask is applied before the crop: moving the crop by one pixel changes which pixels are zeroed."""
    img = np.full((4, 4), 80, np.uint8)
    mask = np.zeros((4, 4), np.uint8)
    mask[1, 1] = 255
    assert prep_host(L, ref.GRAY, img, mask, (0, 0, 2, 2)).tolist() == [[60]]     # (1, 1) is inside
    assert prep_host(L, ref.GRAY, img, mask, (1, 1, 2, 2)).tolist() == [[60]]     # it is the crop's S00
    assert prep_host(L, ref.GRAY, img, mask, (2, 1, 2, 2)).tolist() == [[80]]     # shifted out
    assert prep_host(L, ref.GRAY, img, mask, (1, 2, 2, 2)).tolist() == [[80]]
    assert prep_host(L, ref.GRAY, img, mask, (0, 0, 4, 4)).tolist() == [[60, 80], [80, 80]]


@pytest.mark.parametrize("code", [ref.BGR, ref.RGB])
def test_planted_resize_then_gray(L, code):
    """A block where resize-then-gray and gray-then-resize differ, found by search: the product gives the former."""
    rng = np.random.default_rng(7 + code)
    for _ in range(2000):
        img = rng.integers(0, 256, (2, 2, 3), dtype=np.uint8)
        a = ref.front_prep(img, None, (0, 0, 2, 2), code)
        b = ref.gray_then_half(img, (0, 0, 2, 2), code)
        if a[0, 0] != b[0, 0]:
            break
    else:
        pytest.fail("no block separates the two orders")
    assert abs(int(a[0, 0]) - int(b[0, 0])) == 1
    got = prep_host(L, code, img, None, (0, 0, 2, 2))
    assert got[0, 0] == a[0, 0] and got[0, 0] != b[0, 0]


def test_planted_weights_and_alpha(L):
    """A pure first-byte image: 255 * 1868 for BGR (blue), 255 * 4899 for RGB (red); the alpha byte is not read."""
    img = np.zeros((2, 2, 3), np.uint8)
    img[:, :, 0] = 255
    blue, red = (255 * 1868 + 8192) >> 14, (255 * 4899 + 8192) >> 14
    assert (blue, red) == (29, 76)
    assert prep_host(L, ref.BGR, img, None, (0, 0, 2, 2)).tolist() == [[blue]]
    assert prep_host(L, ref.RGB, img, None, (0, 0, 2, 2)).tolist() == [[red]]
    img4 = np.zeros((2, 2, 4), np.uint8)
    img4[:, :, 0] = 255
    for alpha in (0, 77, 255):
        img4[:, :, 3] = alpha
        assert prep_host(L, ref.BGRA, img4, None, (0, 0, 2, 2)).tolist() == [[blue]]
        assert prep_host(L, ref.RGBA, img4, None, (0, 0, 2, 2)).tolist() == [[red]]


def _bird_host(L, m, so=0, spad=0, do=0, dpad=0):
    h, w, c = m.shape
    s, srs = _laid(m, so, spad)
    drs = w + dpad
    d = np.full(do + h * drs + 8, SENT, np.uint8)
    assert L.orb_bird_mask_host(c, _ptr(s, so), w, h, srs, _ptr(d, do), drs) == 0
    out = np.zeros((h, w), np.uint8)
    keep = np.ones(len(d), bool)
    for y in range(h):
        out[y] = d[do + y * drs:do + y * drs + w]
        keep[do + y * drs:do + y * drs + w] = False
    assert (d[keep] == SENT).all()
    return out


def test_planted_bird_mask_threshold(L):
    """G = 19 -> 0, G = 20 -> 250 (not 255); the other channels do not matter.  One row of 300: the footprint covers
    columns [120, 178) of it (150 - 14.03 - 15 = 120.97 -> 120; 28.07 + 30 = 58.07 -> 58), the planted pixels lie left."""
    for c in (3, 4):
        m = np.zeros((1, 300, c), np.uint8)
        m[0, :, 1] = 200
        m[0, 0, :3] = (255, 19, 255)
        m[0, 1, :3] = (0, 20, 0)
        m[0, 2, 1] = 255
        m[0, 3, :3] = (255, 0, 255)
        out = _bird_host(L, m)[0]
        assert out[:5].tolist() == [0, 250, 250, 0, 250]
        assert out[119] == 250 and not out[120:178].any() and out[178] == 250 and (out[178:] == 250).all()


@pytest.mark.parametrize("w,h", [(160, 200), (64, 64)])
def test_bird_mask_footprint_is_the_existing_rectangle(L, orbgpu_mod, w, h):
    """Over an all-valid mask the output is orb_bird_footprint_mask's rectangle in a 250-filled image: inside the image
    at 160 x 200, clipped at 64 x 64."""
    m = np.full((h, w, 3), 255, np.uint8)
    want = orbgpu_mod.bird_footprint_mask(np.full((h, w), 250, np.uint8))
    x0, y0, x1, y1 = ref.footprint_rect(w, h)
    if (w, h) == (160, 200):
        assert 0 < x0 < x1 < w and 0 < y0 < y1 < h
    else:
        assert (y0, y1) == (0, h) and 0 < x0 < x1 < w      # clipped above and below
    assert (want[y0:y1, x0:x1] == 0).all() and (want == 0).sum() == (x1 - x0) * (y1 - y0)
    assert np.array_equal(_bird_host(L, m, 1, 3, 2, 1), want)
    assert np.array_equal(ref.bird_mask(m), want)


def test_bird_mask_matches_reference(L):
    rng = np.random.default_rng(11)
    for k, (w, h, c) in enumerate([(37, 53, 3), (64, 64, 4), (160, 200, 3), (1, 1, 3), (5, 2, 4)]):
        m = rng.integers(0, 40, (h, w, c), dtype=np.uint8)
        assert np.array_equal(_bird_host(L, m, k % 4, (0, 1, 3)[k % 3], (k + 1) % 4, k % 2), ref.bird_mask(m)), (w, h, c)


# ---- the repository's fisheye fixture ----

@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(GOLDEN, "mask_new_front.npz"))
    keep = np.unpackbits(g["keep_bits"], axis=1)[:, :int(g["shape"][1])].astype(bool)
    assert keep.shape == (1208, 1920)
    return g, keep


@pytest.mark.parametrize("s", [0, 5])
def test_driver_frame_equals_fixture(orbgpu_mod, fx, s):
    """The driver's own geometry: a 1920 x 1208 frame, the reference's camera mask, crop (0, 0, 1900, 800)."""
    from orbgpu.synth import fisheye_driver_frame, synth_frame
    g, keep = fx
    mask = np.where(keep, 0, 255).astype(np.uint8)
    got = orbgpu_mod.front_prep_host(synth_frame(1920, 1208, s), mask, (0, 0, 1900, 800))
    assert got.shape == (400, 950)
    assert np.array_equal(got, fisheye_driver_frame(keep, s)[0])
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(g[f"img_sha256_{s}"])


# ---- argument errors: ORB_ERR_ARG, the destination untouched ----

def test_front_prep_host_errors(L):
    img = np.zeros((8, 12, 3), np.uint8)
    mask = np.zeros((8, 12, 3), np.uint8)
    dst = np.full(64, SENT, np.uint8)

    def call(code=ref.BGR, src=img, sw=12, sh=8, srs=36, m=None, mc=3, mrs=36, cx=0, cy=0, cw=8, ch=4, d=dst, drs=4):
        return L.orb_front_prep_host(code, _ptr(src), sw, sh, srs, _ptr(m), mc, mrs, cx, cy, cw, ch, _ptr(d), drs)

    assert call() == 0 and (dst[:8] == 0).all() and (dst[8:] == SENT).all()      # a 4 x 2 output
    dst[:] = SENT
    bad = [dict(code=4), dict(code=-2), dict(code=7), dict(m=mask, mc=2), dict(m=mask, mc=4), dict(m=mask, mc=0),
           dict(cw=7), dict(ch=3), dict(cw=-2), dict(ch=-2), dict(cx=-1), dict(cy=-1), dict(cx=5), dict(cy=5),
           dict(cw=14), dict(ch=10), dict(sw=8193, srs=3 * 8193), dict(sh=8193), dict(sw=-1), dict(srs=35),
           dict(m=mask, mrs=35), dict(drs=3), dict(src=None), dict(d=None)]
    for kw in bad:
        assert call(**kw) == ARG, kw
        assert (dst == SENT).all(), kw
    assert L.orb_last_error()
    # an empty crop: ORB_OK, nothing touched, NULL arrays accepted
    assert call(cw=0, src=None, d=None) == 0 and call(ch=0) == 0 and (dst == SENT).all()
    # a 1-channel code reads sw bytes a row
    assert call(code=ref.GRAY, srs=12) == 0
    assert call(code=ref.GRAY, srs=11) == ARG
    assert call(code=ref.BGRA, srs=47) == ARG


def test_bird_mask_host_errors(L):
    m = np.zeros((4, 6, 3), np.uint8)
    dst = np.full(64, SENT, np.uint8)

    def call(c=3, src=m, w=6, h=4, srs=18, d=dst, drs=6):
        return L.orb_bird_mask_host(c, _ptr(src), w, h, srs, _ptr(d), drs)

    assert call() == 0
    dst[:] = SENT
    for kw in [dict(c=1), dict(c=2), dict(c=5), dict(w=-1), dict(h=-1), dict(w=4097, srs=3 * 4097, drs=4097),
               dict(h=4097), dict(srs=17), dict(drs=5), dict(src=None), dict(d=None)]:
        assert call(**kw) == ARG, kw
        assert (dst == SENT).all(), kw
    assert call(w=0, src=None, d=None) == 0 and call(h=0) == 0 and (dst == SENT).all()


def test_prep_handle_null_arguments(L):
    """The handle calls that need no GPU to refuse: NULL handles and outputs."""
    w, h = ctypes.c_int(7), ctypes.c_int(7)
    assert L.orb_prep_size(None, ctypes.byref(w), ctypes.byref(h)) == ARG and (w.value, h.value) == (7, 7)
    assert L.orb_prep_source_size(None, ctypes.byref(w), ctypes.byref(h)) == ARG and (w.value, h.value) == (7, 7)
    assert L.orb_prep_create(None, 4, 4, None, 1, 0, 0, 0, 4, 4, None) == ARG          # out NULL
    out = ctypes.c_void_p()
    assert L.orb_prep_create(None, 4, 4, None, 1, 0, 0, 0, 3, 4, ctypes.byref(out)) == ARG and not out   # odd side first
    assert L.orb_prep_create(None, 4, 4, None, 1, 0, 0, 0, 4, 4, ctypes.byref(out)) == ARG and not out   # NULL context
    dst = np.full(16, SENT, np.uint8)
    assert L.orb_front_prep_device(None, None, ref.GRAY, _ptr(dst), 1, 0, 4, _ptr(dst), 0, 2) == ARG
    n = ctypes.c_int(-5)
    assert L.orb_extract_fisheye(None, None, ref.GRAY, _ptr(dst), 4, None, 0, ctypes.byref(n), None) == ARG
    assert n.value == -5 and (dst == SENT).all()
    L.orb_prep_destroy(None)


def test_prep_definitions_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "prep_host_test")
    src = os.path.join(ROOT, "tests", "cpp_prep", "prep_host_test.cc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "prep_def OK" in r.stdout, r.stdout + r.stderr
