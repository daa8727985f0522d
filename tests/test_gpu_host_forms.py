"""GPU: the three host-image entry points (orb_extract, orb_extract_color, orb_extract_rectified) share one body
(extract_host) and no state, and the two kinds of orb_frame creator share one handle layout (frame_alloc).  Everything
is compared byte for byte."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
# a 160 x 120 image holds four pyramid levels of the extractor (a level needs 62 pixels a side)
W, H, LEVELS, NFEAT = 160, 120, 4, 500
RAW_W, RAW_H = 176, 132
CAPACITY = -3   # ORB_ERR_CAPACITY


def _images():
    """Gray A, BGR B (three scenes as its channels) and raw C of another size with the 160 x 120 maps that rectify it
    (a scaling by 1.1 with a mild shear and barrel, a few pixels thrown outside the raw image)."""
    from orbgpu.synth import synth_frame
    A = synth_frame(W, H, 21)
    B = np.ascontiguousarray(np.stack([synth_frame(W, H, 22 + c) for c in range(3)], -1))
    C = synth_frame(RAW_W, RAW_H, 25)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = xx / (W - 1) - 0.5, yy / (H - 1) - 0.5
    r2 = u * u + v * v
    mx = ((u * (1 + 0.1 * r2) + 0.02 * v + 0.5) * (RAW_W - 1) + 0.75).astype(f32)
    my = ((v * (1 + 0.08 * r2) - 0.015 * u + 0.5) * (RAW_H - 1) - 0.5).astype(f32)
    return A, B, C, mx, my


@pytest.fixture(scope="module")
def cases(orbgpu_mod):
    """The images and, computed once on a fresh context through plain orb_extract, what each form must return:
    gray A, the CPU definition's gray of B and the CPU definition's rectified C."""
    A, B, C, mx, my = _images()
    gray_B = orbgpu_mod.to_gray_host(B, orbgpu_mod.COLOR_BGR)
    rect_C = orbgpu_mod.remap_host(C, mx, my)
    assert rect_C.shape == (H, W) and (mx < 0).any() and (my < 0).any()
    fresh = orbgpu_mod.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7)
    try:
        want = {name: fresh(img) for name, img in (("A", A), ("B", gray_B), ("C", rect_C))}
    finally:
        fresh.close()
    for name, (k, d) in want.items():
        assert len(k) > 30, (name, len(k))
    assert len({k.tobytes() for k, _ in want.values()}) == 3   # three different results: a mix-up would show
    return dict(A=A, B=B, C=C, mx=mx, my=my, rect_C=rect_C, want=want)


def _same(got, want):
    return got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("env", [{}, {"ORBGPU_UPLOAD": "1"}], ids=["plain_upload", "streamed_upload"])
def test_host_forms_share_no_state(orbgpu_mod, cases, monkeypatch, env):
    """gray A, colour B, rectified C, gray A, a colour call that fails for capacity, gray A on ONE context: every form
    returns what plain orb_extract returns for the CPU definition's image on a fresh context, whatever ran before it,
    and mvImagePyramid[0] is the image the last call extracted.  With the streamed upload switched on (read at
    orb_create) the gray steps take it, the colour and rectified steps still the plain one; the bytes are the same."""
    from orbgpu import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A, B, want = cases["A"], cases["B"], cases["want"]
    g = orbgpu_mod.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7)
    R = orbgpu_mod.Rectifier(g, cases["mx"], cases["my"])
    try:
        assert R.size == (W, H) and cases["C"].shape == (RAW_H, RAW_W)
        assert _same(g(A), want["A"])                                            # 1
        assert _same(g(B, color=orbgpu_mod.COLOR_BGR), want["B"])                # 2
        assert _same(g(cases["C"], rectify=R), want["C"])                        # 3
        assert np.array_equal(g.mvImagePyramid[0], cases["rect_C"])
        assert _same(g(A), want["A"])                                            # 4
        assert np.array_equal(g.mvImagePyramid[0], A)
        kps = np.full(1, 7, orbgpu_mod.KP_DTYPE)                                 # 5
        desc = np.full((1, 32), 7, np.uint8)
        n = ctypes.c_int(-1)
        st = _lib.lib().orb_extract_color(g.h, orbgpu_mod.COLOR_BGR, ctypes.c_void_p(B.ctypes.data), W, H, B.strides[0],
                                          ctypes.c_void_p(kps.ctypes.data), 1, ctypes.byref(n),
                                          ctypes.c_void_p(desc.ctypes.data))
        assert st == CAPACITY and n.value == len(want["B"][0]) > 1
        assert (desc == 7).all() and kps.tobytes() == np.full(1, 7, orbgpu_mod.KP_DTYPE).tobytes()
        assert _same(g(A), want["A"])                                            # 6
        assert np.array_equal(g.mvImagePyramid[0], A)
    finally:
        R.close()
        g.close()


# ---------------------------------------------------------------- one handle layout

@pytest.fixture(scope="module")
def extraction(orbgpu_mod):
    """One 160 x 120 frame extracted on the device, and its host copy."""
    from orbgpu.synth import synth_frame
    ext = orbgpu_mod.BatchExtractor(NFEAT, W, H, 1, nlevels=LEVELS)
    ext.upload(synth_frame(W, H, 21)[None])
    ext.launch()
    ext.sync()
    k, desc = ext.results(0)
    assert len(k) > 30
    yield ext, k.copy(), desc.copy()
    ext.close()


BOUNDS = (0.0, float(W), 0.0, float(H))


def _identity(orbgpu):
    return orbgpu.distortion(120.0, 121.0, 80.0, 60.0, (0.0, 1.0, 1.0, 1.0))   # k[0] == 0: mvKeysUn = mvKeys


def test_both_creators_lay_out_one_handle(orbgpu_mod, extraction):
    """orb_frame_create_device and orb_frame_create_from_extract (identity distortion) over the same output slots: the
    same count, the same grid (cell_off and the used part of cell_idx), and the same matches from one window search
    whose train side is the handle."""
    ext, k, desc = extraction
    n, d_desc, d_kps = ext.frame_slots(0)
    m = orbgpu_mod.ORBmatcher(0.9, True)
    F = orbgpu_mod.Frame.from_device(ext, n, d_desc, d_kps, bounds=BOUNDS)
    G = orbgpu_mod.Frame.from_extraction(ext, _identity(orbgpu_mod), n, d_desc, d_kps, bounds=BOUNDS)
    try:
        assert len(F) == len(G) == len(k) == n
        (off_f, idx_f), (off_g, idx_g) = F.grid(), G.grid()
        assert off_f[-1] == len(idx_f) > 0
        assert np.array_equal(off_f, off_g) and np.array_equal(idx_f, idx_g)
        # every keypoint searches a window around itself among the frame's own features
        nf, mf = m.window_match_grid(False, desc, k, window=12.0, frame=F)
        ng, mg = m.window_match_grid(False, desc, k, window=12.0, frame=G)
        assert nf == ng > 0 and np.array_equal(mf, mg)
    finally:
        F.close()
        G.close()


def test_both_creators_make_an_empty_handle(orbgpu_mod, extraction):
    ext, _, _ = extraction
    F = orbgpu_mod.Frame.from_device(ext, 0, None, None, bounds=BOUNDS)
    G = orbgpu_mod.Frame.from_extraction(ext, _identity(orbgpu_mod), 0, None, None, bounds=BOUNDS)
    try:
        for X in (F, G):
            off, idx = X.grid()
            assert len(X) == 0 and off.shape == (64 * 48 + 1,) and not off.any() and len(idx) == 0
    finally:
        F.close()
        G.close()
