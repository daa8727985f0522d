"""Inputs of the keyframe-search tests (Fuse, SearchBySim3, the keyframe forms of SearchByProjection), generated on
the CPU from fixed seeds: synthetic keyframes in 640x480 bounds on 8 levels.  tests/test_kf_projection_ref.py checks
that they reach every branch the restatement counts; the GPU tests run them against kf_projection_ref.

A keyframe is kf_projection_ref's dict plus `grid` / `min_xy` for the product; a Fuse target is (kf, pts)."""
import functools

import numpy as np

import kf_projection_ref as ref

f32 = np.float32
BOUNDS = (0.0, 640.0, 0.0, 480.0)
NLEVELS = 8
SCALE = np.ones(NLEVELS, f32)
for _i in range(1, NLEVELS):
    SCALE[_i] = SCALE[_i - 1] * f32(1.2)                         # ORBextractor.cc:431-437
INV_SIGMA2 = (f32(1.0) / (SCALE * SCALE)).astype(f32)            # :439-447
TH = f32(3.0)
# (x, y, kpr) of the three isolated level-0 trains the gate's boundary queries aim at: mono, stereo, stereo with
# mvuRight exactly 0 (the reference tests >= 0)
EDGE_TRAINS = ((2.0, 2.0, -1.0), (20.0, 2.0, 1.0), (40.0, 2.0, 0.0))


def _flip(rng, d, nbits):
    out = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def make_kf(seed, nt, dense=80):
    """nt trains: the three EDGE_TRAINS, a dense cluster of `dense` trains at (500, 100) on levels 6-7 (a window
    there holds more than 64), a sparse pair of clusters (1 and 5 trains), the rest random at x > 60.  A third of the
    descriptors repeat another train's (distance ties across slots).  uright: -1, exactly 0 and positive."""
    from oracle import KP_DTYPE
    rng = np.random.default_rng(seed)
    k = np.zeros(nt, KP_DTYPE)
    ur = np.full(nt, -1, f32)
    desc = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    ne = len(EDGE_TRAINS)
    for j, (x, y, r) in enumerate(EDGE_TRAINS):
        k["x"][j], k["y"][j], k["octave"][j], ur[j] = x, y, 0, r
    a, b = ne, ne + dense
    k["x"][a:b] = 500 + rng.uniform(-9, 9, dense)
    k["y"][a:b] = 100 + rng.uniform(-9, 9, dense)
    k["octave"][a:b] = rng.integers(6, 8, dense)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    for j in range(a, b):
        desc[j] = _flip(rng, base, int(rng.integers(0, 5)) * 4)     # many equal distances to a query made from base
    k["x"][b], k["y"][b], k["octave"][b] = 250.0, 60.0, 2           # a window with exactly one candidate
    c = b + 1
    k["x"][c:c + 5] = 120 + rng.uniform(-2, 2, 5)                   # ... and one with five
    k["y"][c:c + 5] = 300 + rng.uniform(-2, 2, 5)
    k["octave"][c:c + 5] = rng.integers(1, 3, 5)
    d = c + 5
    k["x"][d:] = rng.uniform(60, 630, nt - d)
    k["y"][d:] = rng.uniform(130, 470, nt - d)
    k["octave"][d:] = rng.integers(0, NLEVELS, nt - d)
    k["angle"] = rng.uniform(0, 360, nt).astype(f32)
    kind = rng.integers(0, 10, nt)
    rest = np.arange(nt) >= ne
    ur[rest & (kind >= 5)] = (k["x"] - rng.uniform(0.5, 4, nt).astype(f32))[rest & (kind >= 5)]
    ur[rest & (kind == 4)] = 0.0
    for j in range(d, nt):                                          # repeated descriptors among the random trains
        if rng.random() < 0.33:
            desc[j] = desc[int(rng.integers(d, nt))]
    order = np.concatenate([np.arange(ne), ne + rng.permutation(nt - ne)])   # mix the indices (cells keep index order)
    k, desc, ur = k[order], np.ascontiguousarray(desc[order]), ur[order]
    return dict(desc=desc, kps=k, bounds=BOUNDS, uright=ur, inv_sigma2=INV_SIGMA2, base=base, scale=SCALE)


def _find_v(u, kpx, kpy, ur, kpr, const, above):
    """A float32 v with e2 * 1.0 (level 0) the float32 next to `const` on the wanted side: the largest value not
    above the double constant, or the smallest above it."""
    t = f32(const)
    lo = t if float(t) <= const else np.nextafter(t, f32(0))
    target = np.nextafter(lo, f32(np.inf)) if above else lo
    ex = f32(f32(u) - f32(kpx))
    rest = float(target) - float(ex) * float(ex) - (float(f32(ur) - f32(kpr)) ** 2 if kpr >= 0 else 0.0)
    v0 = f32(kpy + np.sqrt(rest))
    v = np.nextafter(v0, f32(0))
    for _ in range(64):
        v = np.nextafter(v, f32(0))
    for _ in range(200):
        if ref.fuse_e2(u, v, ur, kpx, kpy, kpr)[0] == target:
            return v
        v = np.nextafter(v, f32(np.inf))
    raise AssertionError("no float32 v reaches the boundary value")


def edge_points():
    """Twelve level-0 points (radius 3) whose gate values are the float32 neighbours of 5.99 (mono) and 7.8 (stereo,
    mvuRight 1.0 and exactly 0.0) on each side, at two window offsets: (u, v, ur, the train aimed at, the train
    expected with the gate or -1)."""
    out = []
    for j, (kpx, kpy, kpr) in enumerate(EDGE_TRAINS):
        const = 5.99 if kpr < 0 else 7.8
        for u in (f32(kpx + 2.375), f32(kpx + 2.40625)) if kpr < 0 else (f32(kpx + 2.6875), f32(kpx + 2.71875)):
            ur = f32(kpr + 0.5) if kpr >= 0 else f32(3.0)
            for above in (False, True):
                out.append((u, _find_v(u, kpx, kpy, ur, kpr, const, above), ur, j, -1 if above else j))
    return out


def make_points(seed, kf, nq, edges=(), period=8):
    """nq projected points of a keyframe's trains: near a train (noise below the chi-square gate's reach) with that
    train's descriptor lightly changed, at a predicted level of the train's octave or one above, some at a level that
    excludes it, some far from the projection, some in the dense cluster, some over nothing (the kinds repeat every
    `period` points), and first the gate's boundary points `edges`."""
    rng = np.random.default_rng(seed)
    kps, n = kf["kps"], len(kf["kps"])
    u, v, urr, level = np.zeros(nq, f32), np.zeros(nq, f32), np.zeros(nq, f32), np.zeros(nq, np.int32)
    desc = np.zeros((nq, 32), np.uint8)
    dense = np.flatnonzero((np.abs(kps["x"] - 500) < 9.5) & (np.abs(kps["y"] - 100) < 9.5))
    for i in range(nq):
        if i < len(edges):
            u[i], v[i], urr[i] = edges[i][:3]
            level[i] = 0
            desc[i] = kf["desc"][edges[i][3]]
            continue
        kind = i % period
        t = int(rng.choice(dense)) if kind == 1 else int(rng.integers(len(EDGE_TRAINS), n))
        noise = 6.0 if kind == 2 else 0.8                     # kind 2: beyond the gate at the low levels
        u[i] = kps["x"][t] + rng.uniform(-noise, noise)
        v[i] = kps["y"][t] + rng.uniform(-noise, noise)
        urr[i] = (kf["uright"][t] if kf["uright"][t] >= 0 else u[i] - 2) + rng.uniform(-0.5, 0.5)
        level[i] = min(int(kps["octave"][t]) + int(rng.integers(0, 2)), NLEVELS - 1)
        if kind == 3:
            level[i] = (int(kps["octave"][t]) + 3) % NLEVELS  # the train's octave is outside (level - 1, level)
        if kind == 4 and i % 16 == 4:
            u[i], v[i] = 30.0 + rng.uniform(0, 10), 100.0 + rng.uniform(0, 20)   # nothing there
        desc[i] = _flip(rng, kf["base"] if kind == 1 else kf["desc"][t], int(rng.integers(0, 30)))
    if nq > len(edges) + 2:                                   # the windows with exactly one and five candidates
        one = int(np.flatnonzero((kps["x"] == 250.0) & (kps["y"] == 60.0))[0])
        u[-1], v[-1], level[-1], desc[-1] = 250.5, 60.5, 2, kf["desc"][one]
        u[-2], v[-2], level[-2] = 120.0, 300.0, 2
    radius = (TH * kf["scale"][level]).astype(f32)            # :890 / :1049
    radius[level >= 6] *= f32(1.5)                            # (a larger th at the top levels: wider dense windows)
    return dict(u=u, v=v, ur=urr, level=level, radius=radius, desc=np.ascontiguousarray(desc))


@functools.lru_cache(maxsize=None)
def fuse_targets():
    """The three Fuse targets (300 / 450 / 600 trains, 37 / 130 / 201 points), then one with no points and one with no
    trains."""
    from oracle import KP_DTYPE
    out = []
    e = edge_points()
    for seed, nt, nq, edges, period in ((11, 300, 37, e[:2] + e[4:6], 32), (12, 450, 130, e, 8), (13, 600, 201, e, 8)):
        kf = make_kf(seed, nt)
        out.append((kf, make_points(100 + seed, kf, nq, tuple(edges), period)))
    kf = make_kf(14, 300)
    out.append((kf, make_points(114, kf, 0)))
    empty = dict(desc=np.zeros((0, 32), np.uint8), kps=np.zeros(0, KP_DTYPE), bounds=BOUNDS, uright=np.zeros(0, f32),
                 inv_sigma2=INV_SIGMA2, base=out[0][0]["base"], scale=SCALE)
    pts = make_points(115, out[0][0], 20)
    out.append((empty, pts))
    return out


def window_counts(oracle, kf, pts):
    return [len(oracle.features_in_area(kf["kps"], *kf["bounds"], float(pts["u"][i]), float(pts["v"][i]),
                                        float(pts["radius"][i]), -1, -1)) for i in range(len(pts["u"]))]


@functools.lru_cache(maxsize=None)
def sim3_case():
    """Two keyframes seeing the same scene: KF2's features are KF1's moved by a few pixels with descriptors lightly
    changed (and some changed a lot, so the two directions disagree).  Every feature is a map point projected into
    the other keyframe with noise."""
    rng = np.random.default_rng(21)
    kf1 = make_kf(21, 500)
    n = len(kf1["kps"])
    k2 = kf1["kps"].copy()
    k2["x"] = np.clip(k2["x"] + 4 + rng.uniform(-1, 1, n), 0.5, 639).astype(f32)
    k2["y"] = np.clip(k2["y"] + 3 + rng.uniform(-1, 1, n), 0.5, 479).astype(f32)
    d2 = np.stack([_flip(rng, kf1["desc"][i], int(rng.integers(0, 90))) for i in range(n)])
    perm = rng.permutation(n)
    kf2 = dict(kf1, kps=k2[perm], desc=np.ascontiguousarray(d2[perm]), uright=kf1["uright"][perm])
    inv = np.argsort(perm)                                   # feature i of KF1 is feature inv[i] of KF2

    def project(src, dst, dst_of_src, sel):
        level = np.minimum(dst["kps"]["octave"][dst_of_src[sel]] + rng.integers(0, 2, len(sel)), NLEVELS - 1)
        level = level.astype(np.int32)
        return dict(index=sel.astype(np.int32),
                    u=(dst["kps"]["x"][dst_of_src[sel]] + rng.uniform(-2, 2, len(sel))).astype(f32),
                    v=(dst["kps"]["y"][dst_of_src[sel]] + rng.uniform(-2, 2, len(sel))).astype(f32),
                    level=level, radius=(f32(7.5) * SCALE[level]).astype(f32),
                    desc=np.ascontiguousarray(src["desc"][sel]))
    sel1 = np.sort(rng.choice(n, 330, replace=False))
    sel2 = np.sort(rng.choice(n, 310, replace=False))
    return kf1, kf2, project(kf1, kf2, inv, sel1), project(kf2, kf1, perm, sel2)


def _sequential_case(seed, nt, nq, th, level_above):
    rng = np.random.default_rng(seed)
    kf = make_kf(seed, nt)
    kps = kf["kps"]
    t = rng.integers(len(EDGE_TRAINS), nt, nq)
    t[nq - 60:] = t[:60]                                     # two points on one window: the taken branch
    level = np.minimum(kps["octave"][t] + rng.integers(0, 2, nq), NLEVELS - 1).astype(np.int32)
    level[::9] = (kps["octave"][t[::9]] + 3) % NLEVELS
    angle = kps["angle"][t].astype(f32).copy()
    turned = rng.random(nq) < 0.12                           # some points seen at another in-plane rotation
    angle[turned] = (angle[turned] + f32(100.0) + rng.uniform(0, 120, int(turned.sum())).astype(f32)) % f32(360.0)
    pts = dict(u=(kps["x"][t] + rng.uniform(-1.5, 1.5, nq)).astype(f32),
               v=(kps["y"][t] + rng.uniform(-1.5, 1.5, nq)).astype(f32), level=level,
               radius=(f32(th) * SCALE[level]).astype(f32), angle=angle,
               desc=np.ascontiguousarray(np.stack([_flip(rng, kf["desc"][j], int(rng.integers(0, 40))) for j in t])))
    taken = rng.random(nt) < 0.1
    return pts, kf, taken


@functools.lru_cache(maxsize=None)
def loop_case():
    """SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th = 10) (LoopClosing.cc:375)."""
    return _sequential_case(31, 600, 400, 10.0, 0)


@functools.lru_cache(maxsize=None)
def reloc_case():
    """SearchByProjection(CurrentFrame, pKF, sFound, th = 10, ORBdist = 100) with the rotation check
    (Tracking.cc:2013)."""
    return _sequential_case(32, 600, 400, 10.0, 1) + (100, True)


def product_kf(orbgpu, kf):
    """The keyframe as the Python mirror's wrappers take it."""
    b = kf["bounds"]
    return dict(desc=kf["desc"], kps=kf["kps"], grid=orbgpu.frame_grid(kf["kps"], *b), min_xy=(b[0], b[2]),
                uright=kf["uright"], inv_sigma2=kf["inv_sigma2"])


_EXPECTED = {}


def expected_fuse(oracle, k, chi2):
    """fuse_search of target k, computed once per process and never modified."""
    key = ("fuse", k, bool(chi2))
    if key not in _EXPECTED:
        kf, pts = fuse_targets()[k]
        bi, bd, c = ref.fuse_search(oracle, kf, pts, chi2)
        bi.setflags(write=False)
        bd.setflags(write=False)
        _EXPECTED[key] = (bi, bd, c)
    return _EXPECTED[key]


def expected(oracle, name):
    if name not in _EXPECTED:
        if name == "sim3":
            r = ref.search_by_sim3(oracle, *sim3_case())
        elif name == "loop":
            r = ref.search_kf_scw(oracle, *loop_case())
        else:
            pts, kf, taken, orb_dist, ori = reloc_case()
            r = ref.search_f_kf(oracle, pts, kf, taken, orb_dist, ori)
        for a in r:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _EXPECTED[name] = r
    return _EXPECTED[name]
