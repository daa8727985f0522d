"""GPU: resident map points (orb_points), their projection kernel and the fused searches, against the restatement
tests/frustum_ref.py and against the staged entry points fed with the restatement's visible points."""
import functools

import numpy as np
import pytest

import frustum_cases as fc
import frustum_ref as ref
import kf_projection_cases as kfc
import projection_cases as pc

pytestmark = pytest.mark.gpu
f32 = np.float32
NS = (0, 1, 63, 64, 65, 256, 257, 1031)      # the wave and block edges of k_project_points


@pytest.fixture(scope="module")
def matcher(orbgpu_mod):
    return orbgpu_mod.ORBmatcher(0.8, True)


def _records(orbgpu, mode, cam, arrays, limit, th):
    a = ref.as_array(ref.project(mode, cam, *arrays, view_cos_limit=limit, th=th), orbgpu.POINT_PROJ_DTYPE)
    a.setflags(write=False)
    return a


# ---- (g) orb_project_points against the restatement ----

@functools.lru_cache(maxsize=None)
def _shell():
    """Slots: the planted points, then 1,100 random ones around the general camera."""
    cam = fc.make_camera(3)
    planted = fc.arrays(fc.planted())
    rnd = fc.random_points(17, 1100, cam)
    arrays = tuple(np.concatenate([a, b]) for a, b in zip(planted, rnd))
    rng = np.random.default_rng(1)
    desc = rng.integers(0, 256, (len(arrays[0]), 32), dtype=np.uint8)
    return cam, arrays, desc, len(planted[0])


@pytest.fixture(scope="module")
def shell_points(orbgpu_mod, matcher):
    cam, arrays, desc, _ = _shell()
    mp = orbgpu_mod.MapPoints(matcher, len(desc))
    mp.write(0, *arrays, desc)
    yield mp
    mp.close()


@functools.lru_cache(maxsize=None)
def _shell_reference(mode, planted_cam):
    import orbgpu
    cam, arrays, _, _ = _shell()
    return _records(orbgpu, mode, fc.PLANT_CAM if planted_cam else cam, arrays, 0.5, 3.0)


@pytest.mark.parametrize("mode", [0, 1], ids=["frame", "fuse"])
def test_projection_equals_the_restatement(orbgpu_mod, shell_points, mode):
    cam, arrays, _, nplant = _shell()
    want = _shell_reference(mode, False)
    counts = np.bincount(want["verdict"][nplant:], minlength=6)
    print("verdicts of the random shell:", counts)
    assert (counts[:5] >= 0.05 * (len(want) - nplant)).all(), counts
    cs = fc.cam_struct(orbgpu_mod, cam)
    rng = np.random.default_rng(5 + mode)
    for n in NS:
        ids = rng.integers(0, len(want), n).astype(np.int32)       # out of order, with repeats
        if n >= 63:
            ids[:nplant] = np.arange(nplant)[::-1]
            ids[-1] = ids[0]
        got = shell_points.project(mode, cs, ids, view_cos_limit=0.5, th=3.0)
        for k in ref.FIELDS:
            assert got[k].tobytes() == want[k][ids].tobytes(), (n, k)


@pytest.mark.parametrize("mode", [0, 1], ids=["frame", "fuse"])
@pytest.mark.parametrize("th", [1.0, 3.0])
def test_planted_points_on_the_gpu(orbgpu_mod, shell_points, mode, th):
    cam, arrays, _, nplant = _shell()
    planted = tuple(a[:nplant] for a in arrays)
    want = _records(orbgpu_mod, mode, fc.PLANT_CAM, planted, 0.5, th)
    assert list(want["verdict"]) == [p[5 + mode] for p in fc.planted()]
    got = shell_points.project(mode, fc.cam_struct(orbgpu_mod, fc.PLANT_CAM), np.arange(nplant), 0.5, th)
    for k in ref.FIELDS:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


# ---- (h) orb_search_local_points ----

@functools.lru_cache(maxsize=None)
def _local_case():
    """The second view of projection_cases as the frame (stereo, bounds off the image's); one map point per feature of
    it, 80 repeated (two points on one window), 300 of the random shell (rejected in every way), in mixed order."""
    (_, _, kb, db), _ = pc.views()
    cam = fc.make_camera(8, bounds=pc.BOUNDS)
    rng = np.random.default_rng(21)
    pos, nr, lo, hi, desc = fc.points_on_features(31, cam, kb, db)
    extra = fc.random_points(32, 300, cam)
    arrays = tuple(np.concatenate([a, b]) for a, b in zip((pos, nr, lo, hi), extra))
    desc = np.concatenate([desc, rng.integers(0, 256, (300, 32), dtype=np.uint8)])
    ids = np.concatenate([np.arange(len(desc)), rng.choice(len(kb), 80, replace=False)])
    ids = ids[rng.permutation(len(ids))].astype(np.int32)
    uright = pc._stereo_uright(rng, kb)
    taken = (rng.random(len(kb)) < 0.1).astype(np.uint8)
    return cam, arrays, desc, ids, kb, db, uright, taken


@pytest.fixture(scope="module")
def local_setup(orbgpu_mod, matcher):
    cam, arrays, desc, ids, kb, db, uright, taken = _local_case()
    mp = orbgpu_mod.MapPoints(matcher, 16)          # grows on the first write
    mp.write(0, *arrays, desc)
    frame = orbgpu_mod.Frame(matcher, db, kb, bounds=pc.BOUNDS, uright=uright)
    yield mp, frame
    frame.close()
    mp.close()


def _staged_local(orbgpu, matcher, frame, rec, qdesc, taken, use_uright):
    """orb_search_by_projection_frame fed with the visible records; match_t mapped to positions in ids."""
    q, vis = fc.visible_queries(orbgpu, rec)
    nm, mt = matcher.search_by_projection(orbgpu.PROJ_RATIO_SAME_LEVEL, q, qdesc[vis], frame=frame, t_taken=taken,
                                          use_uright=use_uright, max_dist=100)
    return nm, np.where(mt >= 0, vis[np.maximum(mt, 0)], mt).astype(np.int32)


@pytest.mark.parametrize("th", [1.0, 3.0, 5.0])
@pytest.mark.parametrize("use_uright", [False, True])
@pytest.mark.parametrize("with_taken", [False, True])
def test_search_local_points_equals_the_staged_search(orbgpu_mod, matcher, local_setup, th, use_uright, with_taken):
    mp, frame = local_setup
    cam, arrays, desc, ids, kb, db, uright, taken = _local_case()
    want = _records(orbgpu_mod, 0, cam, tuple(a[ids] for a in arrays), 0.5, th)
    tk = taken if with_taken else None
    want_nm, want_mt = _staged_local(orbgpu_mod, matcher, frame, want, desc[ids], tk, use_uright)
    mt, nm, proj = matcher.SearchLocalPoints(mp, fc.cam_struct(orbgpu_mod, cam), ids, frame, th=th, taken=tk,
                                             use_uright=use_uright)
    print("visible", int((want["verdict"] == 0).sum()), "of", len(ids), "matches", want_nm)
    assert want_nm > 150 and (want["verdict"] != 0).sum() > 150
    assert proj.tobytes() == want.tobytes()
    assert nm == want_nm and np.array_equal(mt, want_mt)
    mt2, nm2, none = matcher.SearchLocalPoints(mp, fc.cam_struct(orbgpu_mod, cam), ids, frame, th=th, taken=tk,
                                               use_uright=use_uright, want_proj=False)
    assert none is None and nm2 == nm and np.array_equal(mt2, mt)


def test_search_local_points_edges(orbgpu_mod, matcher, local_setup):
    mp, frame = local_setup
    cam, arrays, desc, ids, kb, db, uright, taken = _local_case()
    cs = fc.cam_struct(orbgpu_mod, cam)
    all_rec = _records(orbgpu_mod, 0, cam, arrays, 0.5, 3.0)
    rejected = np.flatnonzero(all_rec["verdict"] != 0).astype(np.int32)
    visible = np.flatnonzero(all_rec["verdict"] == 0).astype(np.int32)
    # all points rejected
    mt, nm, proj = matcher.SearchLocalPoints(mp, cs, rejected, frame, th=3.0)
    assert nm == 0 and (mt == -1).all() and proj.tobytes() == all_rec[rejected].tobytes()
    # exactly one visible, between rejected ones
    one = np.concatenate([rejected[:70], visible[5:6], rejected[70:140]]).astype(np.int32)
    want_nm, want_mt = _staged_local(orbgpu_mod, matcher, frame, all_rec[one], desc[one], None, False)
    mt, nm, proj = matcher.SearchLocalPoints(mp, cs, one, frame, th=3.0)
    assert want_nm == 1 and nm == 1 and np.array_equal(mt, want_mt) and (mt == 70).sum() == 1
    # no ids, and a frame with no features
    mt, nm, proj = matcher.SearchLocalPoints(mp, cs, np.zeros(0, np.int32), frame, th=3.0)
    assert nm == 0 and (mt == -1).all() and len(proj) == 0
    empty = orbgpu_mod.Frame(matcher, np.zeros((0, 32), np.uint8), np.zeros(0, orbgpu_mod.KP_DTYPE), bounds=pc.BOUNDS)
    mt, nm, proj = matcher.SearchLocalPoints(mp, cs, ids, empty, th=3.0)
    assert nm == 0 and len(mt) == 0
    empty.close()
    # an id outside [0, capacity) is refused before anything runs
    with pytest.raises(orbgpu_mod.OrbError) as e:
        matcher.SearchLocalPoints(mp, cs, np.array([0, len(mp)], np.int32), frame)
    assert e.value.status == -1 and "id outside [0, capacity)" in str(e.value)
    with pytest.raises(orbgpu_mod.OrbError):
        mp.project(0, cs, np.array([-1], np.int32))


# ---- (i) orb_fuse_search_points ----

@functools.lru_cache(maxsize=None)
def _fuse_case(ntargets):
    """ntargets keyframes of differing sizes with their cameras; each one's points sit on its own features (their
    slots follow one another in one handle); target 1 gets no ids and target 3 an empty frame (when there are that
    many)."""
    kfs, cams, slot0, parts = [], [], [], []
    total = 0
    for k in range(ntargets):
        nt = 0 if k == 3 else 300 + 37 * (k % 5)
        kf = kfc.make_kf(100 + k, max(nt, 120))
        if nt == 0:
            kf = dict(kf, desc=kf["desc"][:0], kps=kf["kps"][:0], uright=kf["uright"][:0])
        cam = fc.make_camera(40 + k)
        src = kfc.make_kf(100 + k, 120) if nt == 0 else kf      # (points for the empty frame still exist)
        pos, nr, lo, hi, desc = fc.points_on_features(60 + k, cam, src["kps"], src["desc"], nflip=4)
        extra = fc.random_points(80 + k, 60, cam)
        arrays = tuple(np.concatenate([a, b]) for a, b in zip((pos, nr, lo, hi), extra))
        desc = np.concatenate([desc, np.random.default_rng(k).integers(0, 256, (60, 32), dtype=np.uint8)])
        kfs.append(kf)
        cams.append(cam)
        slot0.append(total)
        parts.append(arrays + (desc,))
        total += len(desc)
    merged = tuple(np.concatenate([p[j] for p in parts]) for j in range(5))
    idl = []
    for k in range(ntargets):
        n = len(parts[k][4])
        rng = np.random.default_rng(200 + k)
        ids = (slot0[k] + rng.permutation(n)[: n - 13 * (k % 3)]).astype(np.int32)
        idl.append(ids[:0] if k == 1 else ids)
    return kfs, cams, merged, idl


@pytest.mark.parametrize("ntargets", [1, 2, 17])
def test_fuse_search_points_equals_the_staged_search(orbgpu_mod, matcher, ntargets):
    kfs, cams, merged, idl = _fuse_case(ntargets)
    mp = orbgpu_mod.MapPoints(matcher, len(merged[4]))
    mp.write(0, *merged)
    frames = [orbgpu_mod.Frame(matcher, kf["desc"], kf["kps"], bounds=kf["bounds"], uright=kf["uright"]) for kf in kfs]
    th = [3.0 if k % 2 == 0 else 2.5 for k in range(ntargets)]
    targets = [dict(camera=fc.cam_struct(orbgpu_mod, cams[k]), frame=frames[k], inv_sigma2=kfc.INV_SIGMA2, th=th[k],
                    ids=idl[k]) for k in range(ntargets)]
    got = matcher.FuseSearchPoints(mp, targets)
    nfound = 0
    for k in range(ntargets):
        ids = idl[k]
        want = _records(orbgpu_mod, 1, cams[k], tuple(a[ids] for a in merged[:4]), 0.5, th[k])
        q, vis = fc.visible_queries(orbgpu_mod, want)
        (bi, bd), = matcher.project_best_batch(orbgpu_mod.PROJ_GATE_FUSE,
                                               [dict(q=q, qdesc=merged[4][ids][vis], frame=frames[k],
                                                     inv_sigma2=kfc.INV_SIGMA2)])
        want_idx, want_dist = np.full(len(ids), -1, np.int32), np.full(len(ids), -1, np.int32)
        want_idx[vis], want_dist[vis] = bi, bd
        gi, gd, gp = got[k]
        assert np.array_equal(gi, want_idx) and np.array_equal(gd, want_dist), k
        if len(frames[k]) and len(ids):
            assert gp.tobytes() == want.tobytes(), k
            nfound += int((gi >= 0).sum())
        # the same target on its own
        (si, sd, sp), = matcher.FuseSearchPoints(mp, [targets[k]])
        assert np.array_equal(si, gi) and np.array_equal(sd, gd) and sp.tobytes() == gp.tobytes(), k
    print("targets", ntargets, "points with a best train", nfound)
    assert nfound > 60 * min(ntargets, 3)
    for f in frames:
        f.close()
    mp.close()


# ---- (j) orb_points_write ----

def test_points_write_overwrite_growth_and_second_context(orbgpu_mod, matcher):
    cam, arrays, desc, nplant = _shell()
    cs = fc.cam_struct(orbgpu_mod, cam)
    n = 200
    sl = lambda a, b: tuple(x[a:b] for x in arrays)
    mp = orbgpu_mod.MapPoints(matcher, 50)
    assert len(mp) == 50
    mp.write(0, *sl(nplant, nplant + 50), desc[:50])
    mp.write(50, *sl(nplant + 50, nplant + n), desc[50:n])            # grows past the capacity: slots 0..49 stay
    assert len(mp) >= n
    want = _shell_reference(0, False)[nplant:nplant + n]
    ids = np.arange(n, dtype=np.int32)
    assert mp.project(0, cs, ids, 0.5, 3.0).tobytes() == want.tobytes()
    # one slot rewritten with another point: exactly that record changes
    src = nplant + n + 7
    assert want[77].tobytes() != _shell_reference(0, False)[src].tobytes()
    mp.write(77, *sl(src, src + 1), desc[src:src + 1])
    got = mp.project(0, cs, ids, 0.5, 3.0)
    changed = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
    assert changed == [77] and got[77].tobytes() == _shell_reference(0, False)[src].tobytes()
    # a handle created through one context serves another context of the same device
    other = orbgpu_mod._Ctx(500, 1.2, 8, 20, 7, 0)
    assert mp.project(0, cs, ids, 0.5, 3.0, ctx_or_matcher=other).tobytes() == got.tobytes()
    mp.close()
    other.close()


def test_rewritten_descriptor_is_the_one_searched(orbgpu_mod, matcher, local_setup):
    """Overwriting a slot's descriptor changes that point's match and nothing else's."""
    cam, arrays, desc, ids, kb, db, uright, taken = _local_case()
    cs = fc.cam_struct(orbgpu_mod, cam)
    mp = orbgpu_mod.MapPoints(matcher, len(desc))
    mp.write(0, *arrays, desc)
    frame = local_setup[1]
    order = np.arange(len(kb), dtype=np.int32)
    mt0, nm0, proj = matcher.SearchLocalPoints(mp, cs, order, frame, th=3.0)
    slot = int(mt0[mt0 >= 0][10])
    train = int(np.flatnonzero(mt0 == slot)[0])
    mp.write(slot, arrays[0][slot:slot + 1], arrays[1][slot:slot + 1], arrays[2][slot:slot + 1],
             arrays[3][slot:slot + 1], 255 - desc[slot:slot + 1])      # every bit flipped: no train within TH_HIGH
    d2 = desc.copy()
    d2[slot] = 255 - desc[slot]
    want = _records(orbgpu_mod, 0, cam, tuple(a[order] for a in arrays), 0.5, 3.0)
    want_nm, want_mt = _staged_local(orbgpu_mod, matcher, frame, want, d2[order], None, False)
    mt1, nm1, _ = matcher.SearchLocalPoints(mp, cs, order, frame, th=3.0)
    assert nm1 == want_nm and np.array_equal(mt1, want_mt) and mt1[train] != slot
    mp.close()
