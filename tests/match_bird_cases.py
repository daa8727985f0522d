"""Inputs of the SearchByMatchBird tests, generated on the CPU from fixed seeds.  tests/test_match_bird_ref.py checks
that every case reaches the branches it is for (WANT, from the restatement's own counters);
tests/test_gpu_match_bird.py and tests/test_gpu_match_bird_mirror.py run them on the GPU against match_bird_ref.

A keyframe-form case is a dict: form "kf", kf (index, x, y, angle, desc), frame (desc, kps, bounds), r, nnratio,
check_ori, max_dist.  A frame-form case: form "frame", last, cur (desc, kps, bounds), has_mp (or None), window,
nnratio, check_ori.  Descriptors are a few prototypes with some bits flipped, and several queries are made from one
train, so that ratio tests, equal distances and steals happen."""
import functools

import numpy as np

import match_bird_ref as ref

f32 = np.float32
TOPK = 8   # K of orb-slam-birdview_amd/csrc/matcher.hip: the length of the top-k lists the host replay reads


def _flip(rng, d, nbits):
    out = d.copy()
    for b in rng.choice(256, int(nbits), replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _kps(x, y, octave, angle):
    from oracle import KP_DTYPE
    k = np.zeros(len(x), KP_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = np.asarray(x, f32), np.asarray(y, f32), octave, np.asarray(angle, f32)
    return k


def clustered_frame(rng, size, nt, noct, nproto=3, spread=6.0, flips=(4, 40), per_cluster=6):
    """nt birdview keypoints in clusters of about per_cluster (a window holds several candidates), on noct octaves;
    a cluster's descriptors are one prototype with flips[0]..flips[1] bits flipped."""
    ncl = max(1, nt // per_cluster)
    cen = rng.uniform(12, size - 12, (ncl, 2))
    which = rng.integers(0, ncl, nt)
    xy = np.clip(cen[which] + rng.uniform(-spread, spread, (nt, 2)), 0.0, size - 0.01)
    protos = rng.integers(0, 256, (nproto, 32), dtype=np.uint8)
    pc = rng.integers(0, nproto, ncl)
    desc = np.stack([_flip(rng, protos[pc[which[t]]], rng.integers(flips[0], flips[1] + 1)) for t in range(nt)]) \
        if nt else np.zeros((0, 32), np.uint8)
    k = _kps(xy[:, 0], xy[:, 1], rng.integers(0, noct, nt), rng.uniform(0, 360, nt))
    return dict(desc=np.ascontiguousarray(desc, np.uint8), kps=k, bounds=(0.0, float(size), 0.0, float(size)))


def queries_from(rng, frame, nq, noise=3.0, max_flip=16, turned=0.08):
    """nq keyframe map points, each made from a train drawn with replacement: its position plus noise, its descriptor
    with 0..max_flip - 1 bits flipped, its angle (a few turned by 95 degrees); the ids are ascending with gaps."""
    k, d = frame["kps"], frame["desc"]
    src = rng.integers(0, len(k), nq)
    x = (k["x"][src] + rng.uniform(-noise, noise, nq)).astype(f32)
    y = (k["y"][src] + rng.uniform(-noise, noise, nq)).astype(f32)
    desc = np.stack([_flip(rng, d[s], rng.integers(0, max_flip)) for s in src])
    angle = (k["angle"][src] + rng.uniform(-3, 3, nq)).astype(f32)
    t = rng.random(nq) < turned
    angle[t] = (angle[t] + f32(95.0)) % f32(360.0)
    angle = np.mod(angle, f32(360.0)).astype(f32)
    index = np.sort(rng.choice(2 * nq + 3, nq, replace=False)).astype(np.int32)
    return dict(index=index, x=x, y=y, angle=angle, desc=np.ascontiguousarray(desc, np.uint8))


def kf_case(seed, size, nt, nq, r, noct, nnratio, check_ori, max_dist=ref.TH_HIGH, **kw):
    rng = np.random.default_rng(seed)
    frame = clustered_frame(rng, size, nt, noct, **kw)
    return dict(form="kf", kf=queries_from(rng, frame, nq), frame=frame, r=float(r), nnratio=nnratio,
                check_ori=check_ori, max_dist=max_dist)


def second_256_case():
    """Windows of two trains on one octave: one near the query's descriptor, one its complement (distance 256).
    With nnratio 0.3 the second best at 256 decides: best < 76.8 is rejected for best in [77, 100]."""
    rng = np.random.default_rng(31)
    n = 40
    cx, cy = np.meshgrid(np.arange(5) * 50.0 + 30, np.arange(8) * 32.0 + 24)
    cx, cy = cx.ravel(), cy.ravel()
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    near = np.stack([_flip(rng, q[i], 60 + (3 * i) // 2) for i in range(n)])     # distances 60, 61, 63, ..., 118
    far = np.bitwise_not(q)
    x = np.concatenate([cx + 1, cx - 1])
    y = np.concatenate([cy, cy + 1])
    order = rng.permutation(2 * n)
    frame = dict(desc=np.ascontiguousarray(np.concatenate([near, far])[order]),
                 kps=_kps(x[order], y[order], np.zeros(2 * n, np.int32), np.zeros(2 * n)),
                 bounds=(0.0, 288.0, 0.0, 288.0))
    kf = dict(index=np.arange(n, dtype=np.int32) * 2, x=cx.astype(f32), y=cy.astype(f32), angle=np.zeros(n, f32), desc=q)
    return dict(form="kf", kf=kf, frame=frame, r=10.0, nnratio=0.3, check_ori=False, max_dist=ref.TH_HIGH)


def exhaustion_case():
    """A cluster of 20 trains in one window and 14 identical queries on it: each takes the closest train no earlier
    one holds at that distance, so the ninth finds the eight entries of its list inadmissible with more in the
    window (a re-rank on the GPU).  120 more trains and 40 ordinary queries around it."""
    rng = np.random.default_rng(37)
    frame = clustered_frame(rng, 320, 120, 2)
    far = frame["kps"]["x"] > 90                 # keep the cluster's window to itself
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    cd = np.stack([_flip(rng, base, 4 + 2 * j) for j in range(20)])
    ck = _kps(40 + rng.uniform(-7, 7, 20), 40 + rng.uniform(-7, 7, 20), rng.integers(0, 2, 20), np.zeros(20))
    order = rng.permutation(int(far.sum()) + 20)
    frame = dict(desc=np.ascontiguousarray(np.concatenate([frame["desc"][far], cd])[order]),
                 kps=np.concatenate([frame["kps"][far], ck])[order], bounds=frame["bounds"])
    kf = queries_from(rng, frame, 40)
    rep = dict(index=kf["index"][-1] + 1 + np.arange(14, dtype=np.int32), x=np.full(14, 40, f32), y=np.full(14, 40, f32),
               angle=np.zeros(14, f32), desc=np.repeat(base[None], 14, 0))
    order = np.argsort(np.concatenate([rng.random(40), rng.random(14)]), kind="stable")
    kf = {k: np.ascontiguousarray(np.concatenate([kf[k], rep[k]])[order]) for k in kf}
    kf["index"] = np.sort(kf["index"]).astype(np.int32)
    return dict(form="kf", kf=kf, frame=frame, r=15.0, nnratio=1.5, check_ori=False, max_dist=ref.TH_HIGH)


def one_cell_case():
    """Every train inside one grid cell (cells are 4 x 5.33 here), 40 queries on it."""
    rng = np.random.default_rng(41)
    nt = 60
    protos = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    desc = np.stack([_flip(rng, protos[t % 2], rng.integers(4, 41)) for t in range(nt)])
    frame = dict(desc=np.ascontiguousarray(desc), bounds=(0.0, 256.0, 0.0, 256.0),
                 kps=_kps(rng.uniform(102.2, 105.8, nt), rng.uniform(101.5, 106.0, nt), rng.integers(0, 3, nt),
                          rng.uniform(0, 360, nt)))
    return dict(form="kf", kf=queries_from(rng, frame, 40, noise=2.0), frame=frame, r=10.0, nnratio=0.8,
                check_ori=True, max_dist=ref.TH_HIGH)


def border_case():
    """Trains along the four borders and in the corners; queries whose windows leave the grid on each side (some
    centres lie outside the bounds)."""
    rng = np.random.default_rng(43)
    size, per = 300.0, 20
    t = rng.uniform(0, size, (4, per))
    e = rng.uniform(0.0, 6.0, (4, per))
    x = np.concatenate([e[0], size - 0.01 - e[1], t[2], t[3], [0.5, size - 0.5, 0.5, size - 0.5]])
    y = np.concatenate([t[0], t[1], e[2], size - 0.01 - e[3], [0.5, 0.5, size - 0.5, size - 0.5]])
    nt = len(x)
    proto = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.stack([_flip(rng, proto, rng.integers(4, 31)) for _ in range(nt)])
    frame = dict(desc=np.ascontiguousarray(desc), kps=_kps(x, y, rng.integers(0, 4, nt), rng.uniform(0, 360, nt)),
                 bounds=(0.0, size, 0.0, size))
    kf = queries_from(rng, frame, 60, noise=5.0)
    out = np.arange(60) % 3 == 0     # every third centre pushed outward, past the border where it was near one
    kf["x"] = np.where(out & (kf["x"] < 8), kf["x"] - 7, np.where(out & (kf["x"] > size - 8), kf["x"] + 7, kf["x"])).astype(f32)
    kf["y"] = np.where(out & (kf["y"] < 8), kf["y"] - 7, np.where(out & (kf["y"] > size - 8), kf["y"] + 7, kf["y"])).astype(f32)
    return dict(form="kf", kf=kf, frame=frame, r=10.0, nnratio=0.9, check_ori=False, max_dist=ref.TH_HIGH)


def frame_case(seed, size, n, window, has_mp, nnratio=0.9, check_ori=True):
    """The last frame's birdview keypoints are the current frame's moved by a few pixels (some twice), descriptors
    with a few bits flipped, the same octaves; has_mp: "all" | "none" | "mixed" | None (a NULL array)."""
    rng = np.random.default_rng(seed)
    cur = clustered_frame(rng, size, n, 3, flips=(4, 30))
    src = rng.integers(0, n, n)
    k = cur["kps"][src].copy()
    k["x"] = (k["x"] + rng.uniform(-5, 5, n)).astype(f32)
    k["y"] = (k["y"] + rng.uniform(-5, 5, n)).astype(f32)
    k["angle"] = np.mod(k["angle"] + rng.uniform(-3, 3, n).astype(f32), f32(360.0))
    last = dict(desc=np.ascontiguousarray(np.stack([_flip(rng, cur["desc"][s], rng.integers(0, 13)) for s in src])),
                kps=k, bounds=cur["bounds"])
    mp = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "mixed": (rng.random(n) < 0.5).astype(np.uint8),
          None: None}[has_mp]
    return dict(form="frame", last=last, cur=cur, has_mp=mp, window=int(window), nnratio=nnratio, check_ori=check_ori)


# name -> builder; every GPU result must equal reference(case) exactly
CASES = {
    "kf_r10_ori": lambda: kf_case(1, 256, 150, 150, 10, 3, 0.8, True),
    "kf_r15": lambda: kf_case(2, 320, 300, 300, 15, 4, 0.7, False),
    "kf_r20_ori_one_octave": lambda: kf_case(3, 384, 200, 260, 20, 1, 0.9, True),
    "kf_r20_th60": lambda: kf_case(4, 288, 40, 40, 20, 2, 0.8, False, max_dist=60),
    "kf_r_larger_than_frame_ori": lambda: kf_case(5, 256, 120, 60, 500, 3, 0.8, True, nproto=2),
    "kf_second_at_256": second_256_case,
    "kf_exhaustion": exhaustion_case,
    "kf_one_cell_ori": one_cell_case,
    "kf_borders": border_case,
    "frame_w15_all": lambda: frame_case(11, 256, 150, 15, "all"),
    "frame_w20_mixed": lambda: frame_case(12, 320, 300, 20, "mixed"),
    "frame_w15_none": lambda: frame_case(13, 288, 80, 15, "none", check_ori=False),
    "frame_w20_null": lambda: frame_case(14, 384, 120, 20, None),
}
# the counters of match_bird_ref each case must reach (> 0); every counter of ref.COUNTERS appears at least once
WANT = {
    "kf_r10_ori": ("steals", "le_skips", "culled_entries", "culled_entries_on_reset_or_reowned"),
    "kf_r15": ("steals", "le_skips", "different_level_accepts"),
    "kf_r20_ori_one_octave": ("steals", "le_skips", "culled_entries", "exhausted_queries"),
    "kf_r20_th60": ("le_skips",),
    "kf_r_larger_than_frame_ori": ("steals", "le_skips", "different_level_accepts", "culled_entries"),
    "kf_second_at_256": ("seconds_at_256",),
    "kf_exhaustion": ("exhausted_queries", "le_skips"),
    "kf_one_cell_ori": ("steals", "le_skips", "culled_entries"),
    "kf_borders": ("steals", "le_skips"),
    "frame_w15_all": ("birdview_matches",),
    "frame_w20_mixed": ("birdview_matches", "matched_without_map_point"),
    "frame_w15_none": ("birdview_matches", "matched_without_map_point"),
    "frame_w20_null": ("birdview_matches", "matched_without_map_point"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def reference(oracle, c, **kw):
    if c["form"] == "kf":
        a = dict(r=c["r"], nnratio=c["nnratio"], check_ori=c["check_ori"], max_dist=c["max_dist"], topk=TOPK)
        a.update(kw)
        return ref.search_kf_f(oracle, c["kf"], c["frame"], **a)
    return ref.search_frame(oracle, c["cur"], c["last"], c["window"], c["nnratio"], c["check_ori"], c["has_mp"])


_EXPECTED = {}


def expected(oracle, name):
    """reference(case(name)), computed once per process and never modified."""
    if name not in _EXPECTED:
        m, n, c = reference(oracle, case(name))
        m.setflags(write=False)
        _EXPECTED[name] = (m, n, c)
    return _EXPECTED[name]


def run_product(orbgpu, c, **kw):
    """The case through the Python binding: (nmatches, match)."""
    if c["form"] == "kf":
        f, q = c["frame"], c["kf"]
        m = orbgpu.ORBmatcher(kw.pop("nnratio", c["nnratio"]), c["check_ori"])
        a = dict(index=q["index"], pt_x=q["x"], pt_y=q["y"], angle=q["angle"], desc_mp=q["desc"], r=c["r"],
                 desc_bird=f["desc"], kps_bird=f["kps"], grid_bird=orbgpu.frame_grid(f["kps"], *f["bounds"]),
                 max_dist=c["max_dist"])
        a.update(kw)
        return m.SearchByMatchBird(**a)
    cur, last = c["cur"], c["last"]
    m = orbgpu.ORBmatcher(c["nnratio"], c["check_ori"])
    return m.SearchByMatchBirdFrame(last["desc"], last["kps"], c["has_mp"], cur["desc"], cur["kps"],
                                    orbgpu.frame_grid(cur["kps"], *cur["bounds"]), c["window"])
