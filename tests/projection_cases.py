"""Inputs of the projection-gated search tests, generated on the CPU from fixed seeds (the oracle extractor is
bit-exact with the GPU one, so these are the features the product would extract).  tests/test_projection_ref.py checks
that they reach every branch of the reference loops; tests/test_gpu_projection.py and
tests/test_gpu_projection_mirror.py run them on the GPU against projection_ref.

A case is a dict: form ("cflf" | "fmp" | "bird"), the form's arguments for projection_ref (pts, frame, th / r, ...)
and nnratio / check_ori.  reference(oracle, case) evaluates it; the expected results are computed once per process."""
import functools

import numpy as np

import projection_ref as ref

f32 = np.float32
BOUNDS = (3.5, 636.0, 1.0, 470.5)       # a Frame whose undistorted bounds are not the image's (mnMinX > 0)
IMAGE = (0.0, 640.0, 0.0, 480.0)
SCALE = (f32(1.2) ** np.arange(8)).astype(f32)
MBF = 40.0
DX, DY = 5, 3                           # the second view is the first shifted by (DX, DY)


@functools.lru_cache(maxsize=None)
def views():
    """Two 640x480 synth_frame views (the second shifted), 980 features asked of each (the octree returns a few
    more than asked): (kps, desc) x 2, then the
    same for the birdview stream's cv::ORB features."""
    import oracle
    from orbgpu.synth import synth_frame
    a = synth_frame(640, 480, 40)
    b = np.roll(a, (DY, DX), axis=(0, 1))
    ext = oracle.OracleExtractor(980)
    ka, da = ext(a)
    kb, db = ext(b)
    bird = oracle.OracleCvORB(800)
    bka, bda = bird.extract(a)
    bkb, bdb = bird.extract(b)
    return (ka.copy(), da.copy(), kb.copy(), db.copy()), (bka.copy(), bda.copy(), bkb.copy(), bdb.copy())


def _stereo_uright(rng, kps, frac=3):
    """mvuRight on every frac-th train: x minus a disparity, mostly small, sometimes far off the projections'."""
    n = len(kps)
    ur = np.full(n, -1, f32)
    sel = np.arange(n) % frac == 0
    disp = np.where(rng.random(n) < 0.8, rng.uniform(0.5, 4.0, n), rng.uniform(30, 60, n))
    ur[sel] = np.maximum(kps["x"][sel] - disp[sel].astype(f32), f32(0.5))
    return ur


def _projected(rng, ka, da, noise, dup):
    """The first view's features as map points projected into the second (shift + noise), plus `dup` repeated
    projections at the end (two map points landing on one window: the taken / overwrite branches)."""
    n = len(ka)
    sel = np.concatenate([np.arange(n), rng.choice(n, dup, replace=False)])
    u = (ka["x"][sel] + DX + rng.uniform(-noise, noise, len(sel))).astype(f32)
    v = (ka["y"][sel] + DY + rng.uniform(-noise, noise, len(sel))).astype(f32)
    return sel, u, v, np.ascontiguousarray(da[sel])


def cflf_case(seed, th, b_mono, check_ori, forward=False, backward=False):
    (ka, da, kb, db), _ = views()
    rng = np.random.default_rng(seed)
    sel, u, v, desc = _projected(rng, ka, da, 2.0, 60)
    angle = ka["angle"][sel].astype(f32).copy()
    turned = rng.random(len(sel)) < 0.05          # a few map points seen at another in-plane rotation
    angle[turned] = (angle[turned] + f32(95.0)) % f32(360.0)
    observed = np.ones(len(sel), bool)
    if not b_mono:
        observed = rng.random(len(sel)) >= 0.2    # a fifth: temporal points of UpdateLastFrame (no observations)
    pts = dict(u=u, v=v, invzc=rng.uniform(0.01, 0.1, len(sel)).astype(f32), octave=ka["octave"][sel].astype(np.int32),
               angle=angle, observed=observed, desc=desc)
    cf = dict(desc=db, kps=kb, bounds=BOUNDS, scale_factors=SCALE, mbf=MBF,
              uright=None if b_mono else _stereo_uright(rng, kb), taken=rng.random(len(kb)) < 0.05)
    return dict(form="cflf", pts=pts, frame=cf, th=float(th), b_mono=b_mono, check_ori=check_ori, forward=forward,
                backward=backward, nnratio=0.9)


def fmp_case(seed, th, nnratio=0.8, bounds=BOUNDS):
    (ka, da, kb, db), _ = views()
    rng = np.random.default_rng(seed)
    sel, u, v, desc = _projected(rng, ka, da, 1.0, 80)
    level = np.clip(ka["octave"][sel] + rng.integers(-1, 2, len(sel)), 0, 7).astype(np.int32)   # predicted levels 0..7
    view_cos = np.where(rng.random(len(sel)) < 0.5, f32(0.9995), f32(0.99)).astype(f32)
    view_cos[:4] = [0.998, np.nextafter(f32(0.998), f32(1)), np.nextafter(f32(0.998), f32(0)), 1.0]
    disp = rng.uniform(0.5, 4.0, len(sel)).astype(f32)
    pts = dict(proj_x=u, proj_y=v, proj_xr=(u - disp).astype(f32), level=level, view_cos=view_cos, desc=desc)
    frame = dict(desc=db, kps=kb, bounds=bounds, scale_factors=SCALE, uright=_stereo_uright(rng, kb),
                 taken=rng.random(len(kb)) < 0.1)
    return dict(form="fmp", pts=pts, frame=frame, th=float(th), nnratio=nnratio)


def bird_case(seed, r, nnratio=0.8):
    _, (ka, da, kb, db) = views()
    rng = np.random.default_rng(seed)
    sel, x, y, desc = _projected(rng, ka, da, 2.0, 60)
    frame = dict(desc=db, kps=kb, bounds=IMAGE, taken=rng.random(len(kb)) < 0.1)
    return dict(form="bird", pts=dict(x=x, y=y, desc=desc), frame=frame, r=float(r), nnratio=nnratio)


def _flip(rng, d, nbits):
    out = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def synthetic_frame(rng, clusters, nrandom=150, octave=0):
    """Keypoints in chosen places: clusters = [(cx, cy, half, count)], then nrandom keypoints away from them (x > 320).
    Descriptors: each cluster's are one random descriptor with 4..60 bits flipped (so a query made from it finds many
    candidates below TH_HIGH); returns (kps, desc, the clusters' base descriptors)."""
    from oracle import KP_DTYPE
    xs, ys, ds, bases = [], [], [], []
    for cx, cy, half, count in clusters:
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        bases.append(base)
        xs += (cx + rng.uniform(-half, half, count)).tolist()
        ys += (cy + rng.uniform(-half, half, count)).tolist()
        ds += [_flip(rng, base, int(rng.integers(4, 61))) for _ in range(count)]
    xs += rng.uniform(330, 630, nrandom).tolist()
    ys += rng.uniform(150, 470, nrandom).tolist()
    ds += list(rng.integers(0, 256, (nrandom, 32), dtype=np.uint8))
    k = np.zeros(len(xs), KP_DTYPE)
    k["x"], k["y"], k["octave"] = np.array(xs, f32), np.array(ys, f32), octave
    k["angle"] = rng.uniform(0, 360, len(xs)).astype(f32)
    order = rng.permutation(len(xs))   # grid cells hold their keypoints in index order: mix the indices
    return k[order], np.ascontiguousarray(np.array(ds, np.uint8)[order]), bases


def exhaustion_case(form):
    """Twelve identical queries on one window of 24 candidates, all below TH_HIGH of the query: each takes the
    best train left, so the ninth finds its eight listed trains taken with more in the window (a re-rank)."""
    rng = np.random.default_rng(11)
    k, d, bases = synthetic_frame(rng, [(100.0, 100.0, 8.0, 24)])
    n = 12
    qd = np.ascontiguousarray(np.repeat(bases[0][None], n, 0))
    frame = dict(desc=d, kps=k, bounds=IMAGE, scale_factors=SCALE, mbf=MBF, uright=None, taken=None)
    if form == "cflf":
        pts = dict(u=np.full(n, 100, f32), v=np.full(n, 100, f32), invzc=np.full(n, 0.05, f32),
                   octave=np.zeros(n, np.int32), angle=np.zeros(n, f32), observed=np.ones(n, bool), desc=qd)
        return dict(form="cflf", pts=pts, frame=frame, th=12.0, b_mono=True, check_ori=False, forward=False,
                    backward=False, nnratio=0.9)
    return dict(form="bird", pts=dict(x=np.full(n, 100, f32), y=np.full(n, 100, f32), desc=qd), frame=frame, r=12.0,
                nnratio=1.5)


def lanes_case():
    """The shapes at which a row-per-query mapping and its reductions can go wrong: 37 queries (no multiple of 16),
    windows holding no candidate, exactly one, a few, and more than 64 (80 in one cluster), interleaved so that one
    wavefront's four rows differ.  CF/LF form, mono, all trains at octave 0 (levels (-1, 1), r = th)."""
    rng = np.random.default_rng(5)
    k, d, bases = synthetic_frame(rng, [(100.0, 100.0, 9.0, 80), (250.0, 60.0, 3.0, 1), (60.0, 300.0, 6.0, 5)],
                                  nrandom=120)
    spots = [(100.0, 100.0, 0), (250.0, 60.0, 1), (60.0, 300.0, 2), (250.0, 300.0, 0)]   # the last: nothing there
    n = 37
    which = np.arange(n) % 4
    u = np.array([spots[w][0] for w in which], f32)
    v = np.array([spots[w][1] for w in which], f32)
    qd = np.ascontiguousarray(np.stack([_flip(rng, bases[spots[w][2]], 3) for w in which]))
    pts = dict(u=u, v=v, invzc=np.full(n, 0.05, f32), octave=np.zeros(n, np.int32), angle=np.zeros(n, f32),
               observed=np.ones(n, bool), desc=qd)
    frame = dict(desc=d, kps=k, bounds=IMAGE, scale_factors=SCALE, mbf=MBF, uright=None, taken=None)
    return dict(form="cflf", pts=pts, frame=frame, th=10.0, b_mono=True, check_ori=False, forward=False,
                backward=False, nnratio=0.9)


def window_counts(oracle, case):
    """Candidates per query of a CF/LF case's windows (before the taken / stereo gates)."""
    p, f = case["pts"], case["frame"]
    out = []
    for i in range(len(p["u"])):
        o = int(p["octave"][i])
        r = f32(case["th"]) * f["scale_factors"][o]
        out.append(len(oracle.features_in_area(f["kps"], *f["bounds"], float(p["u"][i]), float(p["v"][i]), float(r),
                                               o - 1, o + 1)))
    return out


def level_case():
    """The CF/LF form looking forward and backward over a stereo frame (levels (oct, -1) and (0, oct))."""
    return [cflf_case(21, 7, False, True, forward=True), cflf_case(22, 15, False, False, backward=True)]


# name -> builder; the parity cases of the three forms (every GPU result must equal reference(case) exactly)
CASES = {
    "cflf_mono_th7_ori": lambda: cflf_case(1, 7, True, True),
    "cflf_mono_th15": lambda: cflf_case(2, 15, True, False),
    "cflf_stereo_th15_ori": lambda: cflf_case(3, 15, False, True),
    "cflf_stereo_th7": lambda: cflf_case(4, 7, False, False),
    "cflf_forward_th7_ori": lambda: level_case()[0],
    "cflf_backward_th15": lambda: level_case()[1],
    "fmp_th1": lambda: fmp_case(5, 1),
    "fmp_th3": lambda: fmp_case(6, 3),
    "fmp_th5": lambda: fmp_case(7, 5, nnratio=0.7),
    "fmp_th3_image_bounds": lambda: fmp_case(8, 3, bounds=IMAGE),
    "bird_r10": lambda: bird_case(9, 10),
    "bird_r25": lambda: bird_case(10, 25, nnratio=0.6),
}
SPECIAL = {
    "exhaustion_best": lambda: exhaustion_case("cflf"),
    "exhaustion_ratio": lambda: exhaustion_case("bird"),
    "lanes": lanes_case,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or SPECIAL[name])()


def reference(oracle, c):
    if c["form"] == "cflf":
        return ref.search_cf_lf(oracle, c["pts"], c["frame"], c["th"], c["b_mono"], c["check_ori"], c["forward"],
                                c["backward"])
    if c["form"] == "fmp":
        return ref.search_f_mappoints(oracle, c["pts"], c["frame"], c["th"], c["nnratio"])
    return ref.search_bird(oracle, c["pts"], c["frame"], c["r"], c["nnratio"])


_EXPECTED = {}


def expected(oracle, name):
    """reference(case(name)), computed once per process and never modified."""
    if name not in _EXPECTED:
        m, n, c = reference(oracle, case(name))
        m.setflags(write=False)
        _EXPECTED[name] = (m, n, c)
    return _EXPECTED[name]


def run_product(orbgpu, c):
    """The case through the Python binding's wrapper of its reference function: (nmatches, match_t)."""
    p, f = c["pts"], c["frame"]
    b = f["bounds"]
    grid = orbgpu.frame_grid(f["kps"], *b)
    if c["form"] == "cflf":
        m = orbgpu.ORBmatcher(c["nnratio"], c["check_ori"])
        return m.SearchByProjection_CF_LF(p["u"], p["v"], p["invzc"], p["octave"], p["angle"], p["observed"], p["desc"],
                                          f["scale_factors"], f["mbf"], c["th"], c["b_mono"], f["desc"], f["kps"], grid,
                                          f["uright"], f["taken"], (b[0], b[2]), c["forward"], c["backward"])
    m = orbgpu.ORBmatcher(c["nnratio"], True)
    if c["form"] == "fmp":
        return m.SearchByProjection_F_MapPoints(p["proj_x"], p["proj_y"], p["proj_xr"], p["level"], p["view_cos"],
                                                p["desc"], f["scale_factors"], c["th"], f["desc"], f["kps"], grid,
                                                f["uright"], f["taken"], (b[0], b[2]))
    return m.SearchByProjectionBird(p["x"], p["y"], p["desc"], c["r"], f["desc"], f["kps"], grid, f["taken"])
