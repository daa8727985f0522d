"""Resident Frame handles (orb_frame): the grid k_frame_grid builds on the GPU equals orbgpu.frame_grid() array for
array (tests/test_gpu_matcher.py pins frame_grid() to the oracle), and every grid search on a handle gives the outputs
of its host-pointer entry point on the same inputs, exactly.  The search inputs are those of tests/projection_cases.py,
kf_projection_cases.py and match_bird_cases.py."""
import ctypes

import numpy as np
import pytest

import kf_projection_cases as kc
import match_bird_cases as mc
import projection_cases as pc

pytestmark = pytest.mark.gpu
f32 = np.float32
IMAGE = (0.0, 640.0, 0.0, 480.0)


@pytest.fixture(scope="module")
def m(orbgpu_mod):
    return orbgpu_mod.ORBmatcher(0.8, True)


def _kps(orbgpu, x, y):
    k = np.zeros(len(x), orbgpu.KP_DTYPE)
    k["x"], k["y"] = np.asarray(x, f32), np.asarray(y, f32)
    return k


def _desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _grid_equal(orbgpu, m, k, bounds):
    """Frame.grid() over keypoints k against frame_grid(k, *bounds); returns cell_off."""
    F = orbgpu.Frame(m, np.zeros((len(k), 32), np.uint8), k, bounds=bounds)
    try:
        off, idx = F.grid()
    finally:
        F.close()
    inv_w, inv_h, want_off, want_idx = orbgpu.frame_grid(k, *bounds)
    assert F.inv == (inv_w, inv_h)
    assert off.dtype == want_off.dtype and np.array_equal(off, want_off)
    assert np.array_equal(idx, want_idx), np.flatnonzero(idx != want_idx)[:8]
    return off


# ---------------------------------------------------------------- the grid

@pytest.mark.parametrize("n", [1000, 2000])
@pytest.mark.parametrize("bounds", [pc.BOUNDS, IMAGE])
def test_grid_random_keypoints(orbgpu_mod, m, n, bounds):
    rng = np.random.default_rng(n)
    off = _grid_equal(orbgpu_mod, m, _kps(orbgpu_mod, rng.uniform(-6, 646, n), rng.uniform(-6, 486, n)), bounds)
    assert 0.9 * n < off[-1] < n   # some fall outside


def test_grid_birdview_inverses_given(orbgpu_mod, m):
    """The birdview grid: origin 0 and the inverse cell sizes given directly."""
    rng = np.random.default_rng(3)
    n, size = 800, 384.0
    k = _kps(orbgpu_mod, rng.uniform(0, size, n), rng.uniform(0, size, n))
    inv_w, inv_h, want_off, want_idx = orbgpu_mod.frame_grid(k, 0.0, size, 0.0, size)
    F = orbgpu_mod.Frame(m, _desc(rng, n), k, inv=(inv_w, inv_h))
    off, idx = F.grid()
    F.close()
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)


@pytest.mark.parametrize("n", [0, 1])
def test_grid_tiny(orbgpu_mod, m, n):
    off = _grid_equal(orbgpu_mod, m, _kps(orbgpu_mod, [100.0] * n, [100.0] * n), IMAGE)
    assert off[-1] == n


def test_grid_rounding_edges_and_outside(orbgpu_mod, m):
    """Keypoints whose (x - min_x) * inv_w is exactly k + 0.5, -0.5, -0.49, 63.49 and 63.5 (y: 47.49, 47.5, 48), and
    keypoints outside on every side.  Bounds (0, 64, 0, 48): both inverses are 1, so the products are the
    coordinates themselves."""
    b = (0.0, 64.0, 0.0, 48.0)
    xs = [0.5, 1.5, 2.5, 7.5, 62.5, -0.5, -0.49, -0.3, 63.49, 63.5, 64.0, 10.0, 10.0, 10.0, 10.0, 10.0, 10.0]
    ys = [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 0.5, -0.5, -0.49, 47.49, 47.5, 48.0]
    xs += [-3.0, 70.0, 20.0, 20.0, -3.0, 70.0]   # outside: left, right, above, below, two corners
    ys += [20.0, 20.0, -3.0, 52.0, -3.0, 52.0]
    k = _kps(orbgpu_mod, xs, ys)
    off = _grid_equal(orbgpu_mod, m, k, b)
    inside = {0: (1, 5), 1: (2, 5), 2: (3, 5), 3: (8, 5), 4: (63, 5), 6: (0, 5), 7: (0, 5), 8: (63, 5), 11: (10, 1),
              13: (10, 0), 14: (10, 47)}
    assert off[-1] == len(inside)
    F = orbgpu_mod.Frame(m, np.zeros((len(k), 32), np.uint8), k, bounds=b)
    off, idx = F.grid()
    F.close()
    for i, (ix, iy) in inside.items():
        c = ix * 48 + iy
        assert i in idx[off[c]:off[c + 1]].tolist(), (i, ix, iy)
    # the same edges through a scaled grid: x = min_x + (k + 0.5) / inv_w where that product is exact
    b2 = (8.0, 8.0 + 128.0, 4.0, 4.0 + 96.0)   # inverses 0.5
    k2 = _kps(orbgpu_mod, [8 + 2 * v for v in (0.5, 1.5, -0.5, 63.5, 63.25)], [4 + 2 * v for v in (47.5, 0.5, 1.0, 2.0, 47.25)])
    off = _grid_equal(orbgpu_mod, m, k2, b2)
    assert off[-1] == 2   # (2, 1) and (63, 47)


@pytest.mark.parametrize("n", [1, 64, 65, 300, 2500])
def test_grid_all_in_one_cell(orbgpu_mod, m, n):
    """One cell holds every keypoint: the segment is ordered by one lane's count, by a wave's, and (2,500) rebuilt by the
    whole workgroup."""
    rng = np.random.default_rng(n)
    k = _kps(orbgpu_mod, 100 + rng.uniform(-3, 3, n), 200 + rng.uniform(-3, 3, n))
    off = _grid_equal(orbgpu_mod, m, k, IMAGE)
    c = 10 * 48 + 20
    assert off[c] == 0 and off[c + 1] == n


def test_grid_mixed_long_and_short_cells(orbgpu_mod, m):
    """Two cells above the workgroup threshold (1,024) among ordinary ones."""
    rng = np.random.default_rng(8)
    x = np.concatenate([100 + rng.uniform(-3, 3, 1500), 400 + rng.uniform(-3, 3, 1100), rng.uniform(0, 640, 1400)])
    y = np.concatenate([200 + rng.uniform(-3, 3, 1500), 300 + rng.uniform(-3, 3, 1100), rng.uniform(0, 480, 1400)])
    p = rng.permutation(len(x))
    _grid_equal(orbgpu_mod, m, _kps(orbgpu_mod, x[p], y[p]), IMAGE)


def test_grid_indices_beyond_16_bits(orbgpu_mod, m):
    n = 70000
    rng = np.random.default_rng(70)
    off = _grid_equal(orbgpu_mod, m, _kps(orbgpu_mod, rng.uniform(0, 640, n), rng.uniform(0, 480, n)), IMAGE)
    # x in [635, 640) rounds to column 64 and y in [475, 480) to row 48: 5/640 + 5/480 = 1.8 % fall outside
    assert 68000 < off[-1] < 69500


# ---------------------------------------------------------------- the searches

def _frame_of(orbgpu, m, f, uright=True):
    """The resident Frame of a case's train frame dict (desc, kps, bounds, uright)."""
    return orbgpu.Frame(m, f["desc"], f["kps"], bounds=f["bounds"], uright=f.get("uright") if uright else None)


def _run_projection(orbgpu, c, resident):
    """pc.run_product, and the same call with the trains as a resident Frame."""
    if not resident:
        return pc.run_product(orbgpu, c)
    p, f = c["pts"], c["frame"]
    if c["form"] == "cflf":
        mm = orbgpu.ORBmatcher(c["nnratio"], c["check_ori"])
        F = _frame_of(orbgpu, mm, f)
        r = mm.SearchByProjection_CF_LF(p["u"], p["v"], p["invzc"], p["octave"], p["angle"], p["observed"], p["desc"],
                                        f["scale_factors"], f["mbf"], c["th"], c["b_mono"], taken_cf=f["taken"],
                                        bForward=c["forward"], bBackward=c["backward"], frame=F)
    elif c["form"] == "fmp":
        mm = orbgpu.ORBmatcher(c["nnratio"], True)
        F = _frame_of(orbgpu, mm, f)
        r = mm.SearchByProjection_F_MapPoints(p["proj_x"], p["proj_y"], p["proj_xr"], p["level"], p["view_cos"],
                                              p["desc"], f["scale_factors"], c["th"], taken_f=f["taken"], frame=F)
    else:
        mm = orbgpu.ORBmatcher(c["nnratio"], True)
        F = _frame_of(orbgpu, mm, f, uright=False)
        r = mm.SearchByProjectionBird(p["x"], p["y"], p["desc"], c["r"], taken_bird=f["taken"], frame=F)
    F.close()
    return r


# BEST and RATIO_SAME_LEVEL; uright present (stereo, fmp) and absent; taken present and absent (the exhaustion
# cases); check_ori on; queries with blocks == 0 (the stereo CF/LF cases' temporal points); the replay's re-rank
# (exhaustion_*: twelve queries contending for one window).  The view cases are about 1,040 queries x 990 trains.
PROJ = ["cflf_mono_th7_ori", "cflf_stereo_th15_ori", "cflf_stereo_th7", "cflf_forward_th7_ori", "fmp_th3",
        "fmp_th3_image_bounds", "bird_r10", "exhaustion_best", "exhaustion_ratio", "lanes"]


@pytest.mark.parametrize("name", PROJ)
def test_projection_on_a_handle_equals_host_pointers(orbgpu_mod, name):
    c = pc.case(name)
    n0, m0 = _run_projection(orbgpu_mod, c, False)
    n1, m1 = _run_projection(orbgpu_mod, c, True)
    assert n1 == n0 and np.array_equal(m1, m0), (n0, n1, np.flatnonzero(m0 != m1)[:8])
    if name.startswith("exhaustion"):
        assert n0 == 12
    if name == "cflf_stereo_th7":
        assert (~c["pts"]["observed"]).sum() > 50   # blocks == 0 queries


def _random_case(orbgpu, seed, nq, nt):
    """nq queries x nt trains with random descriptors near their trains', windows of 12 px on a 640x480 grid."""
    rng = np.random.default_rng(seed)
    k = _kps(orbgpu, rng.uniform(0, 640, nt), rng.uniform(0, 480, nt))
    k["octave"] = rng.integers(0, 4, nt)
    k["angle"] = rng.uniform(0, 360, nt)
    d = _desc(rng, nt)
    t = rng.integers(0, nt, nq)
    q = np.zeros(nq, orbgpu.PROJ_QUERY_DTYPE)
    q["u"], q["v"] = k["x"][t] + rng.uniform(-2, 2, nq), k["y"][t] + rng.uniform(-2, 2, nq)
    q["r"], q["min_level"], q["max_level"] = 12.0, -1, -1
    q["ur"], q["ur_tol"] = q["u"] - 2.0, 12.0
    q["angle"] = k["angle"][t]
    q["blocks"] = rng.random(nq) < 0.8
    qd = d[t] ^ (rng.random((nq, 32)) < 0.05).astype(np.uint8)
    ur = np.where(rng.random(nt) < 0.4, k["x"] - rng.uniform(0.5, 4, nt), -1).astype(f32)
    return q, np.ascontiguousarray(qd), d, k, ur, rng.random(nt) < 0.1


@pytest.mark.parametrize("nq,nt", [(300, 500), (1000, 1000)])
@pytest.mark.parametrize("mode", [0, 1])
def test_projection_core_random(orbgpu_mod, nq, nt, mode):
    mm = orbgpu_mod.ORBmatcher(0.8, True)
    q, qd, d, k, ur, taken = _random_case(orbgpu_mod, nq + mode, nq, nt)
    grid = orbgpu_mod.frame_grid(k, *IMAGE)
    F = orbgpu_mod.Frame(mm, d, k, bounds=IMAGE, uright=ur)
    for t_ur, t_tk in ((ur, taken), (None, None), (ur, None), (None, taken)):
        a = mm.search_by_projection(mode, q, qd, d, k, grid, t_ur, t_tk)
        b = mm.search_by_projection(mode, q, qd, t_taken=t_tk, frame=F, use_uright=t_ur is not None)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        assert a[0] > nq // 4
    F.close()


@pytest.mark.parametrize("level0_only", [0, 1])
@pytest.mark.parametrize("centres", [False, True])
def test_window_match_on_a_handle(orbgpu_mod, m, level0_only, centres):
    (ka, da, kb, db), _ = pc.views()
    rng = np.random.default_rng(5)
    cen = None
    if centres:
        cen = np.stack([ka["x"] + pc.DX + rng.uniform(-2, 2, len(ka)), ka["y"] + pc.DY + rng.uniform(-2, 2, len(ka))], 1)
        cen = cen.astype(f32)
    b = pc.BOUNDS
    grid = orbgpu_mod.frame_grid(kb, *b)
    F = orbgpu_mod.Frame(m, db, kb, bounds=b)
    w = 30.0 if centres else 60.0
    a = m.window_match_grid(level0_only, da, ka, db, kb, grid, w, cen, (b[0], b[2]))
    r = m.window_match_grid(level0_only, da, ka, window=w, centres=cen, frame=F)
    F.close()
    assert a[0] == r[0] and np.array_equal(a[1], r[1])
    assert a[0] > 20


@pytest.mark.parametrize("n1,n2", [(0, 50), (40, 0), (0, 0)])
def test_window_match_with_nothing_on_one_side(orbgpu_mod, m, n1, n2):
    """No queries, or an empty handle: the early return gives what orb_window_match_grid gives (all -1, 0)."""
    rng = np.random.default_rng(n1 + n2)
    k1 = _kps(orbgpu_mod, rng.uniform(0, 640, n1), rng.uniform(0, 480, n1))
    k2 = _kps(orbgpu_mod, rng.uniform(0, 640, n2), rng.uniform(0, 480, n2))
    d1, d2 = _desc(rng, n1), _desc(rng, n2)
    F = orbgpu_mod.Frame(m, d2, k2, bounds=IMAGE)
    a = m.window_match_grid(0, d1, k1, d2, k2, orbgpu_mod.frame_grid(k2, *IMAGE), 50.0)
    b = m.window_match_grid(0, d1, k1, window=50.0, frame=F)
    F.close()
    assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1]) and len(b[1]) == n1 and (b[1] == -1).all()


@pytest.mark.parametrize("name", ["kf_r10_ori", "kf_r20_ori_one_octave", "kf_exhaustion", "kf_one_cell_ori"])
def test_match_bird_on_a_handle(orbgpu_mod, name):
    c = mc.case(name)
    f, q = c["frame"], c["kf"]
    mm = orbgpu_mod.ORBmatcher(c["nnratio"], c["check_ori"])
    inv_w, inv_h, _, _ = orbgpu_mod.frame_grid(f["kps"], *f["bounds"])
    F = orbgpu_mod.Frame(mm, f["desc"], f["kps"], inv=(inv_w, inv_h))
    a = mc.run_product(orbgpu_mod, c)
    b = mm.SearchByMatchBird(q["index"], q["x"], q["y"], q["angle"], q["desc"], c["r"], max_dist=c["max_dist"], frame=F)
    F.close()
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("gate", [0, 1])
def test_project_best_on_handles(orbgpu_mod, m, gate):
    """Three targets: one ordinary, one with nq == 0, one whose frame is empty."""
    tg = [kc.fuse_targets()[i] for i in (1, 3, 4)]
    assert len(tg[1][1]["u"]) == 0 and len(tg[2][0]["kps"]) == 0
    host = [orbgpu_mod._kf_target(kc.product_kf(orbgpu_mod, kf), pts) for kf, pts in tg]
    frames = [orbgpu_mod.Frame(m, kf["desc"], kf["kps"], bounds=kf["bounds"], uright=kf["uright"]) for kf, _ in tg]
    res = [orbgpu_mod._kf_target(dict(frame=F, inv_sigma2=kf["inv_sigma2"]), pts) for F, (kf, pts) in zip(frames, tg)]
    a = m.project_best_batch(gate, host)
    b = m.project_best_batch(gate, res)
    for F in frames:
        F.close()
    for (ai, ad), (bi, bd) in zip(a, b):
        assert np.array_equal(ai, bi) and np.array_equal(ad, bd)
    assert (a[0][0] >= 0).sum() > 20 and (a[2][0] == -1).all()


def test_one_handle_many_searches_and_a_second_context(orbgpu_mod):
    """A handle searched three times with different queries, then from a matcher that owns another context on the
    same device: every result is the fresh host-pointer call's."""
    mm = orbgpu_mod.ORBmatcher(0.8, True)
    q, qd, d, k, ur, taken = _random_case(orbgpu_mod, 77, 300, 500)
    grid = orbgpu_mod.frame_grid(k, *IMAGE)
    F = orbgpu_mod.Frame(mm, d, k, bounds=IMAGE, uright=ur)
    rng = np.random.default_rng(1)
    for i in range(3):
        sel = rng.permutation(len(q))[: 200 + 40 * i]
        a = mm.search_by_projection(0, q[sel], qd[sel], d, k, grid, ur, taken)
        b = mm.search_by_projection(0, q[sel], qd[sel], t_taken=taken, frame=F, use_uright=True)
        assert a[0] == b[0] > 0 and np.array_equal(a[1], b[1])
    other = orbgpu_mod.ORBmatcher(0.8, True)
    other._ctx = orbgpu_mod._Ctx(1000, 1.2, 8, 20, 7, 0)   # its own context
    try:
        a = mm.search_by_projection(1, q, qd, d, k, grid, ur, taken)
        b = other.search_by_projection(1, q, qd, t_taken=taken, frame=F, use_uright=True)
        assert a[0] == b[0] > 0 and np.array_equal(a[1], b[1])
    finally:
        F.close()
        other._ctx.close()


def test_frame_from_the_extraction_batch(orbgpu_mod, m):
    """Two 320x240 frames through BatchExtractor; a Frame from frame 1's device slots has frame_grid()'s grid of the
    downloaded keypoints, and a window match of frame 0 against it equals orb_window_match_grid on the downloads."""
    from orbgpu.synth import synth_frame
    W, H = 320, 240
    ext = orbgpu_mod.BatchExtractor(500, W, H, 2)
    a = synth_frame(W, H, 7)
    ext.upload(np.stack([a, np.roll(a, (2, 3), axis=(0, 1))]))
    ext.launch()
    ext.sync()
    (k0, d0), (k1, d1) = ext.results(0), ext.results(1)
    b = (0.0, float(W), 0.0, float(H))
    n, d_desc, d_kps = ext.frame_slots(1)
    assert n == len(k1) > 200
    F = orbgpu_mod.Frame.from_device(ext, n, d_desc, d_kps, bounds=b)
    try:
        off, idx = F.grid()
        grid = orbgpu_mod.frame_grid(k1, *b)
        assert np.array_equal(off, grid[2]) and np.array_equal(idx, grid[3])
        want = m.window_match_grid(0, d0, k0, d1, k1, grid, 20.0)
        got = m.window_match_grid(0, d0, k0, window=20.0, frame=F)
        assert want[0] == got[0] > 20 and np.array_equal(want[1], got[1])
    finally:
        F.close()
        ext.close()


# ---------------------------------------------------------------- argument errors

def test_create_argument_errors(orbgpu_mod, m):
    from orbgpu import _lib
    L = _lib.lib()
    k = _kps(orbgpu_mod, [10.0, 20.0], [10.0, 20.0])
    d = np.zeros((2, 32), np.uint8)
    nan, inf = float("nan"), float("inf")

    def create(fn, n, desc, kps, g):
        out = ctypes.c_void_p(0xdead)
        st = getattr(L, fn)(m._ctx.h, n, desc, kps, None, *g, ctypes.byref(out))
        assert out.value == 0xdead   # untouched
        return st

    ok = (0.0, 0.0, 0.1, 0.1)
    for fn in ("orb_frame_create", "orb_frame_create_device"):
        assert create(fn, -1, d.ctypes.data, k.ctypes.data, ok) == -1
        assert create(fn, 2, None, k.ctypes.data, ok) == -1
        assert create(fn, 2, d.ctypes.data, None, ok) == -1
        for g in ((0.0, 0.0, 0.0, 0.1), (0.0, 0.0, 0.1, -1.0), (0.0, 0.0, nan, 0.1), (0.0, 0.0, 0.1, inf),
                  (nan, 0.0, 0.1, 0.1), (0.0, -inf, 0.1, 0.1)):
            assert create(fn, 2, d.ctypes.data, k.ctypes.data, g) == -1, g
    for bad in (nan, inf):
        for field in ("x", "y"):
            kb = k.copy()
            kb[field][1] = bad
            assert create("orb_frame_create", 2, d.ctypes.data, kb.ctypes.data, ok) == -1


def test_search_argument_errors_leave_outputs_untouched(orbgpu_mod, m):
    from orbgpu import _lib
    L = _lib.lib()
    q, qd, d, k, ur, taken = _random_case(orbgpu_mod, 9, 20, 50)
    F = orbgpu_mod.Frame(m, d, k, bounds=IMAGE)   # no uright
    out = np.full(50, 7, np.int32)
    nm = ctypes.c_int(7)

    def proj(mode=0, max_dist=100, frame=F.h, use_ur=0, queries=q):
        return L.orb_search_by_projection_frame(m._ctx.h, mode, 0.8, 1, max_dist, len(queries), queries.ctypes.data,
                                                qd.ctypes.data, frame, None, use_ur, out.ctypes.data, ctypes.byref(nm))

    assert proj() == 0
    out[:] = 7
    nm.value = 7
    qbad = q.copy()
    qbad["u"][3] = np.nan
    qneg = q.copy()
    qneg["r"][0] = -1
    for kw in (dict(mode=2), dict(max_dist=257), dict(max_dist=-1), dict(frame=None), dict(use_ur=1), dict(queries=qbad),
               dict(queries=qneg)):
        assert proj(**kw) == -1, kw
        assert (out == 7).all() and nm.value == 7, kw
    with pytest.raises(orbgpu_mod.OrbError):
        m.search_by_projection(0, q, qd, frame=F, use_uright=True)
    with pytest.raises(AssertionError):   # neither form of the train side, and both
        m.search_by_projection(0, q, qd)
    with pytest.raises(AssertionError):
        m.search_by_projection(0, q, qd, d, k, orbgpu_mod.frame_grid(k, *IMAGE), frame=F)
    with pytest.raises(AssertionError):
        m.window_match_grid(0, qd, k[:20], window=10.0)
    m12 = np.full(20, 7, np.int32)
    assert L.orb_window_match_frame(m._ctx.h, 0.8, 1, 0, 20, qd.ctypes.data, k.ctypes.data, None, 10.0, None,
                                    m12.ctypes.data, ctypes.byref(nm)) == -1
    xy = np.zeros((20, 2), f32)
    assert L.orb_search_by_match_bird_resident(m._ctx.h, 0.8, 0, 300, 10.0, 20, None, xy.ctypes.data, None,
                                               qd.ctypes.data, F.h, out.ctypes.data, ctypes.byref(nm)) == -1
    assert L.orb_search_by_match_bird_resident(m._ctx.h, 0.8, 0, 100, float("nan"), 20, None, xy.ctypes.data, None,
                                               qd.ctypes.data, F.h, out.ctypes.data, ctypes.byref(nm)) == -1
    bi = np.full(20, 7, np.int32)
    T = _lib.OrbProjFrameTarget(20, q.ctypes.data, qd.ctypes.data, None, None, 0, bi.ctypes.data, bi.ctypes.data)
    assert L.orb_project_best_frames(m._ctx.h, 0, 1, ctypes.addressof(T)) == -1
    T.frame = F.h
    assert L.orb_project_best_frames(m._ctx.h, 1, 1, ctypes.addressof(T)) == -1   # gate FUSE without inv_sigma2
    assert L.orb_project_best_frames(m._ctx.h, 5, 1, ctypes.addressof(T)) == -1
    assert (m12 == 7).all() and (out == 7).all() and (bi == 7).all() and nm.value == 7
    F.close()


def test_handle_of_another_device_is_refused(orbgpu_mod):
    if orbgpu_mod.device_count() < 2:
        pytest.skip("one GPU")
    m0, m1 = orbgpu_mod.ORBmatcher(0.8, True, device=0), orbgpu_mod.ORBmatcher(0.8, True, device=1)
    q, qd, d, k, ur, taken = _random_case(orbgpu_mod, 9, 20, 50)
    F = orbgpu_mod.Frame(m1, d, k, bounds=IMAGE)
    with pytest.raises(orbgpu_mod.OrbError):
        m0.search_by_projection(0, q, qd, frame=F)
    F.close()
