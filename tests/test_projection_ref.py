"""CPU: the test-side restatement of the projection-gated searches (tests/projection_ref.py) on hand-made
known-answer inputs, the equivalence the product's host replay rests on (running two-smallest update == first two of
the (dist, position) order), the reach of the GPU tests' inputs (tests/projection_cases.py), and the argument checks
of orb_search_by_projection that run before any GPU work."""
import ctypes

import numpy as np
import pytest

import projection_cases as pc
import projection_ref as ref

f32 = np.float32


def _desc(nbits):
    """A descriptor at Hamming distance nbits from the all-zero one."""
    d = np.zeros(32, np.uint8)
    for b in range(nbits):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def _frame(oracle_mod, trains, **extra):
    """trains: (x, y, octave, distance to the zero descriptor, uright, taken, angle)."""
    k = np.zeros(len(trains), oracle_mod.KP_DTYPE)
    for i, t in enumerate(trains):
        k["x"][i], k["y"][i], k["octave"][i], k["angle"][i] = t[0], t[1], t[2], t[6] if len(t) > 6 else 0
    return dict(desc=np.stack([_desc(t[3]) for t in trains]), kps=k, bounds=pc.IMAGE, scale_factors=pc.SCALE,
                mbf=pc.MBF, uright=np.array([t[4] for t in trains], f32), taken=np.array([t[5] for t in trains], bool),
                **extra)


def _fmp_pts(points):
    """points: (x, y, xr, level, view_cos); zero descriptors."""
    a = np.array(points, np.float64).reshape(-1, 5)
    return dict(proj_x=a[:, 0].astype(f32), proj_y=a[:, 1].astype(f32), proj_xr=a[:, 2].astype(f32),
                level=a[:, 3].astype(np.int32), view_cos=a[:, 4].astype(f32), desc=np.zeros((len(a), 32), np.uint8))


def _cflf_pts(points):
    """points: (u, v, octave, angle, observed); zero descriptors, invzc 0.05."""
    a = np.array(points, np.float64).reshape(-1, 5)
    return dict(u=a[:, 0].astype(f32), v=a[:, 1].astype(f32), invzc=np.full(len(a), 0.05, f32),
                octave=a[:, 2].astype(np.int32), angle=a[:, 3].astype(f32), observed=a[:, 4] != 0,
                desc=np.zeros((len(a), 32), np.uint8))


def _only(c, **want):
    assert c == {**{k: 0 for k in ref.COUNTERS}, **want}, c


def test_kat_stereo_gate_and_levels_minus1_0(oracle_mod):
    # level 0, th 1, viewCos 1: r = 2.5, levels (-1, 0): checked, nothing below, octave 1 above
    fr = _frame(oracle_mod, [(101, 100, 0, 10, 200.0, 0), (100, 101, 0, 30, -1.0, 0), (99, 100, 1, 5, -1.0, 0)])
    m, n, c = ref.search_f_mappoints(oracle_mod, _fmp_pts([(100, 100, 100, 0, 1.0)]), fr, 1.0, 0.8)
    assert m.tolist() == [-1, 0, -1] and n == 1
    _only(c, stereo_rejections=1)
    # the same train within the tolerance (|100 - 102| <= 2.5) wins
    fr["uright"][0] = 102.0
    m, n, c = ref.search_f_mappoints(oracle_mod, _fmp_pts([(100, 100, 100, 0, 1.0)]), fr, 1.0, 0.8)
    assert m.tolist() == [0, -1, -1] and n == 1
    _only(c)


def test_kat_ratio_same_level_and_different_level(oracle_mod):
    same = _frame(oracle_mod, [(101, 100, 0, 40, -1.0, 0), (100, 101, 0, 45, -1.0, 0)])
    m, n, c = ref.search_f_mappoints(oracle_mod, _fmp_pts([(100, 100, 0, 0, 1.0)]), same, 1.0, 0.8)
    assert m.tolist() == [-1, -1] and n == 0      # 40 > 0.8 * 45 at equal levels
    _only(c, ratio_rejections_same_level=1)
    m, n, c = ref.search_f_mappoints(oracle_mod, _fmp_pts([(100, 100, 0, 0, 1.0)]), same, 1.0, 0.9)
    assert m.tolist() == [0, -1] and n == 1       # 40 <= 0.9 * 45
    _only(c)
    # level 1: levels (0, 1); the second best sits on the other level, so the ratio is not applied
    diff = _frame(oracle_mod, [(101, 100, 0, 40, -1.0, 0), (100, 101, 1, 45, -1.0, 0)])
    m, n, c = ref.search_f_mappoints(oracle_mod, _fmp_pts([(100, 100, 0, 1, 1.0)]), diff, 1.0, 0.8)
    assert m.tolist() == [0, -1] and n == 1
    _only(c, accepted_different_level_despite_ratio=1)
    # a lone candidate: bestLevel2 stays -1, bestDist2 256
    lone = _frame(oracle_mod, [(101, 100, 0, 100, -1.0, 0)])
    m, n, c = ref.search_f_mappoints(oracle_mod, _fmp_pts([(100, 100, 0, 0, 1.0)]), lone, 1.0, 0.1)
    assert m.tolist() == [0] and n == 1
    lone["desc"][0] = _desc(101)
    assert ref.search_f_mappoints(oracle_mod, _fmp_pts([(100, 100, 0, 0, 1.0)]), lone, 1.0, 0.1)[1] == 0   # > TH_HIGH


def test_kat_radius_by_viewing_cos(oracle_mod):
    # a train 3 px away: inside 4.0 (viewCos <= 0.998), outside 2.5 (viewCos > 0.998); th 2 doubles both
    fr = _frame(oracle_mod, [(103, 100, 0, 10, -1.0, 0)])
    for vc, th, hit in [(0.99, 1.0, True), (0.9995, 1.0, False), (0.9995, 2.0, True), (0.998, 1.0, False)]:
        # float(0.998f) = 0.99800002... > 0.998: the narrow window
        n = ref.search_f_mappoints(oracle_mod, _fmp_pts([(100, 100, 0, 0, vc)]), fr, th, 0.8)[1]
        assert n == int(hit), (vc, th)


def test_kat_taken_and_zero_observation_overwrite(oracle_mod):
    fr = _frame(oracle_mod, [(101, 100, 0, 10, -1.0, 0), (100, 101, 0, 30, -1.0, 0), (99, 100, 0, 5, -1.0, 1)])
    # query 0 has no observations: train 0 stays open and query 1 overwrites it (both count); query 1 blocks, so
    # query 2 skips train 0 and takes train 1; train 2 was taken from the start (three skips)
    pts = _cflf_pts([(100, 100, 0, 0, 0), (100, 100, 0, 0, 1), (100, 100, 0, 0, 1)])
    m, n, c = ref.search_cf_lf(oracle_mod, pts, fr, 7.0, True, False)
    assert m.tolist() == [1, 2, -1] and n == 3
    _only(c, zero_observation_overwrites=1, taken_skips=3 + 1)


def test_kat_level_rule_corners(oracle_mod):
    fr = _frame(oracle_mod, [(101, 100, 5, 10, -1.0, 0), (100, 101, 3, 30, -1.0, 0), (99, 100, 2, 50, -1.0, 0)])
    # forward at octave 0: (0, -1) checks nothing, the octave-5 train is a candidate
    m, n, _ = ref.search_cf_lf(oracle_mod, _cflf_pts([(100, 100, 0, 0, 1)]), fr, 7.0, False, False, b_forward=True)
    assert m.tolist() == [0, -1, -1]
    # forward at octave 3: (3, -1): octaves 3 and up
    m, n, _ = ref.search_cf_lf(oracle_mod, _cflf_pts([(100, 100, 3, 0, 1)]), fr, 7.0, False, False, b_forward=True)
    assert m.tolist() == [0, -1, -1]
    # backward at octave 3: (0, 3): the octave-5 train is out
    m, n, _ = ref.search_cf_lf(oracle_mod, _cflf_pts([(100, 100, 3, 0, 1)]), fr, 7.0, False, False, b_backward=True)
    assert m.tolist() == [-1, 0, -1]
    # backward at octave 2: (0, 2)
    m, n, _ = ref.search_cf_lf(oracle_mod, _cflf_pts([(100, 100, 2, 0, 1)]), fr, 7.0, False, False, b_backward=True)
    assert m.tolist() == [-1, -1, 0]
    # neither (and bMono overrides both flags): (oct - 1, oct + 1) = (3, 5) at octave 4
    for kw in ({}, {"b_forward": True}):
        m, n, _ = ref.search_cf_lf(oracle_mod, _cflf_pts([(100, 100, 4, 0, 1)]), fr, 7.0, True, False, **kw)
        assert m.tolist() == [0, -1, -1]
    # octave 0 without a direction: (-1, 1) is checked (max_level >= 0): nothing here is at octave <= 1
    m, n, _ = ref.search_cf_lf(oracle_mod, _cflf_pts([(100, 100, 0, 0, 1)]), fr, 7.0, True, False)
    assert n == 0


def test_kat_stereo_gate_cf_lf(oracle_mod):
    # ur = u - mbf * invzc = 100 - 40 * 0.05 = 98; radius 7: uright 110 is out, 104 is in
    fr = _frame(oracle_mod, [(101, 100, 0, 10, 110.0, 0), (100, 101, 0, 30, 104.0, 0)])
    m, n, c = ref.search_cf_lf(oracle_mod, _cflf_pts([(100, 100, 0, 0, 1)]), fr, 7.0, False, False)
    assert m.tolist() == [-1, 0] and n == 1
    _only(c, stereo_rejections=1)


def test_kat_rotation_cull(oracle_mod):
    # five matches with rotations 0, 0, 90, 180, 270: bins 0 (twice), 3, 6, 9; the fourth bin is culled
    xs = [50, 150, 250, 350, 450]
    rots = [0, 0, 90, 180, 270]
    fr = _frame(oracle_mod, [(x + 1, 100, 0, 10, -1.0, 0, 10.0) for x in xs])
    pts = _cflf_pts([(x, 100, 0, 10.0 + r, 1) for x, r in zip(xs, rots)])
    assert [oracle_mod.rot_bin(10.0 + r, 10.0) for r in rots] == [0, 0, 3, 6, 9]
    m, n, c = ref.search_cf_lf(oracle_mod, pts, fr, 7.0, True, True)
    assert m.tolist() == [0, 1, 2, 3, -2] and n == 4
    _only(c, rotation_culls=1)
    m, n, c = ref.search_cf_lf(oracle_mod, pts, fr, 7.0, True, False)
    assert m.tolist() == [0, 1, 2, 3, 4] and n == 5
    # an overwritten train entered in two culled bins is reset once and decrements twice (:1460-1464 has no guard)
    fr2 = _frame(oracle_mod, [(x + 1, 100, 0, 10, -1.0, 0, 10.0) for x in xs[:4]])
    pts2 = _cflf_pts([(50, 100, 0, 10, 1), (150, 100, 0, 10, 1), (250, 100, 0, 10, 1), (250, 100, 0, 10, 1),
                      (250, 100, 0, 10, 1), (350, 100, 0, 100, 0), (350, 100, 0, 190, 1)])
    m, n, c = ref.search_cf_lf(oracle_mod, pts2, fr2, 7.0, True, True)
    # bin 0 holds trains 0, 1, 2 (queries 3 and 4 find train 2 taken and nothing else); bins 3 and 6 hold train 3 once
    # each and both survive as second and third maxima
    assert m.tolist() == [0, 1, 2, 6] and n == 5 and c["zero_observation_overwrites"] == 1 and c["rotation_culls"] == 0


def test_two_smallest_by_dist_position_equals_running_update():
    """The host replay takes the first two admissible entries of a list sorted by (dist, position) for bestDist /
    bestLevel / bestIdx / bestDist2 / bestLevel2; the reference keeps running minima (:102-114).  Equal on random
    lists full of ties, including distances of 256 (which can never replace the initial 256)."""
    rng = np.random.default_rng(3)
    for trial in range(3000):
        n = int(rng.integers(0, 12))
        hi = [4, 8, 40][trial % 3]
        dists = rng.integers(0, hi, n).tolist()
        if trial % 5 == 0:
            dists = [256 if rng.random() < 0.4 else d for d in dists]
        levels = rng.integers(0, 3, n).tolist()
        assert ref.running_two_smallest(dists, levels) == ref.sorted_two_smallest(dists, levels), (dists, levels)


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_gpu_inputs_give_enough_matches(oracle_mod, name):
    c = pc.case(name)
    nq = len(c["pts"]["desc"])
    nt = len(c["frame"]["kps"])
    m, n, cnt = pc.expected(oracle_mod, name)
    print(name, "queries", nq, "trains", nt, "matches", n, cnt)
    assert 500 <= nt <= 1000 and nq % 16 != 0
    assert n >= 50
    assert int((m >= 0).sum()) >= 50


def test_gpu_inputs_reach_every_branch(oracle_mod):
    """Every counter is driven by the forms that have the branch: the stereo gate and the taken set in all three
    stereo-capable forms' cases, the overwrite by a map point without observations and the rotation cull in the
    CF/LF form, the two ratio outcomes in the two RATIO forms."""
    tot = {}
    for name in pc.CASES:
        form = pc.case(name)["form"]
        for k, v in pc.expected(oracle_mod, name)[2].items():
            tot[form, k] = tot.get((form, k), 0) + v
    print(tot)
    for form, keys in [("cflf", ["stereo_rejections", "taken_skips", "zero_observation_overwrites", "rotation_culls"]),
                       ("fmp", ["stereo_rejections", "taken_skips", "ratio_rejections_same_level",
                                "accepted_different_level_despite_ratio"]),
                       ("bird", ["taken_skips", "ratio_rejections_same_level",
                                 "accepted_different_level_despite_ratio"])]:
        for k in keys:
            assert tot[form, k] >= 1, (form, k)
    for k in ref.COUNTERS:
        assert sum(v for (f, kk), v in tot.items() if kk == k) >= 1, k
    # each stereo CF/LF case on its own reaches the gate, the taken set and the overwrite
    for name in ("cflf_stereo_th15_ori", "cflf_stereo_th7"):
        c = pc.expected(oracle_mod, name)[2]
        assert min(c["stereo_rejections"], c["taken_skips"], c["zero_observation_overwrites"]) >= 1, (name, c)
    assert pc.expected(oracle_mod, "cflf_stereo_th15_ori")[2]["rotation_culls"] >= 1
    assert pc.expected(oracle_mod, "cflf_mono_th7_ori")[2]["rotation_culls"] >= 1


def test_special_inputs_have_their_shapes(oracle_mod):
    for name in ("exhaustion_best", "exhaustion_ratio"):
        c = pc.case(name)
        m, n, cnt = pc.expected(oracle_mod, name)
        assert len(c["pts"]["desc"]) == 12 and n == 12 and sorted(m[m >= 0].tolist()) == list(range(12))
        # the ninth query skips at least eight taken trains that rank before its match
        assert cnt["taken_skips"] == sum(range(12))
    c = pc.case("exhaustion_best")
    assert min(pc.window_counts(oracle_mod, c)) >= 20
    lanes = pc.case("lanes")
    counts = pc.window_counts(oracle_mod, lanes)
    assert len(counts) % 16 != 0 and 0 in counts and 1 in counts and max(counts) > 64
    assert len(set(counts[:4])) == 4   # the four rows of the first wavefront all differ
    assert pc.expected(oracle_mod, "lanes")[1] >= 10


# ---- orb_search_by_projection's argument checks (before the context is looked at: no GPU needed) ----

def _call(orbgpu_mod, mode=0, max_dist=100, q=None, off=None, idx=None, ctx=None, nt=10):
    from orbgpu import _lib
    L = _lib.lib()
    desc = np.zeros((10, 32), np.uint8)
    k = np.zeros(10, orbgpu_mod.KP_DTYPE)
    qq = np.zeros(3, orbgpu_mod.PROJ_QUERY_DTYPE) if q is None else q
    qq["r"] = np.where(qq["r"] == 0, 5.0, qq["r"])
    good = np.zeros(64 * 48 + 1, np.int32)
    good[5:] = 10
    off = good if off is None else off
    idx = np.arange(10, dtype=np.int32) if idx is None else idx
    g = _lib.OrbFrameGrid(0.0, 0.0, 0.1, 0.1, off.ctypes.data, idx.ctypes.data)
    match = np.zeros(10, np.int32)
    nm = ctypes.c_int(-7)
    st = L.orb_search_by_projection(ctx, mode, 0.8, 1, max_dist, len(qq), qq.ctypes.data, desc.ctypes.data, nt,
                                    desc.ctypes.data, k.ctypes.data, None, None, g, match.ctypes.data, ctypes.byref(nm))
    return st, L.orb_last_error().decode()


def test_null_context_is_an_argument_error(orbgpu_mod):
    assert _call(orbgpu_mod) == (-1, "NULL context")


def test_argument_errors_before_any_gpu_work(orbgpu_mod):
    assert _call(orbgpu_mod, mode=2) == (-1, "orb_search_by_projection: unknown mode")
    assert _call(orbgpu_mod, mode=-1)[0] == -1
    for md in (-1, 257):
        assert _call(orbgpu_mod, max_dist=md) == (-1, "orb_search_by_projection: max_dist outside [0, 256]")
    assert _call(orbgpu_mod, max_dist=256) == (-1, "NULL context")
    assert _call(orbgpu_mod, max_dist=0) == (-1, "NULL context")
    for field, val in [("u", np.nan), ("v", np.inf), ("r", np.nan), ("r", np.inf), ("r", -1.0), ("u", -np.inf)]:
        q = np.zeros(3, orbgpu_mod.PROJ_QUERY_DTYPE)
        q[field][1] = val
        assert _call(orbgpu_mod, q=q) == (-1, "orb_search_by_projection: query window not finite or radius negative")
    good = np.zeros(64 * 48 + 1, np.int32)
    good[5:] = 10
    bad = good.copy()
    bad[0] = 1
    assert _call(orbgpu_mod, off=bad) == (-1, "orb_search_by_projection: grid cell_off[0] != 0")
    bad = good.copy()
    bad[100] = 3
    assert _call(orbgpu_mod, off=bad) == (-1, "orb_search_by_projection: grid cell_off decreases")
    idx = np.arange(10, dtype=np.int32)
    idx[7] = 10
    assert _call(orbgpu_mod, idx=idx) == (-1, "orb_search_by_projection: grid index out of range")
    idx[7] = -1
    assert _call(orbgpu_mod, idx=idx) == (-1, "orb_search_by_projection: grid index out of range")
    # an index equal to a smaller nt is out of range too
    assert _call(orbgpu_mod, nt=9)[1] == "orb_search_by_projection: grid index out of range"


def test_grid_is_checked_before_the_query_values(orbgpu_mod):
    """The Frame grid is checked with the other pointers, ahead of the per-query values: a call with a malformed CSR
    and a non-finite query reports the CSR."""
    q = np.zeros(3, orbgpu_mod.PROJ_QUERY_DTYPE)
    q["u"][1] = np.nan
    bad = np.zeros(64 * 48 + 1, np.int32)
    bad[5:] = 10
    bad[100] = 3
    assert _call(orbgpu_mod, q=q, off=bad) == (-1, "orb_search_by_projection: grid cell_off decreases")
    assert _call(orbgpu_mod, q=q, max_dist=257) == (-1, "orb_search_by_projection: max_dist outside [0, 256]")
