"""A toy MapPoint graph for the replay rule of INTEGRATION.md: LocalMapping::SearchInNeighbors (LocalMapping.cc:495-500,
Fuse(pKFi, vpMapPointMatches) per target keyframe) and LoopClosing::SearchAndFuse (LoopClosing.cc:591-612,
Fuse(pKF, Scw, mvpLoopMapPoints, 4, vpReplacePoints), then Replace per point) with the search moved ahead of the loop.

The search of (target, point) reads the point's projection (fixed here) and descriptor and the keyframe's features.
Inside and between the Fuse calls only the graph changes; of its changes only Replace reaches the search, through
ComputeDistinctiveDescriptors() on the surviving point.  So the batched replay walks targets and points in the
reference's order, applies isBad / IsInKeyFrame / GetMapPoint / Observations at replay time, and for a point whose
descriptor bytes differ from those the batched search saw takes the single-point search with the current descriptor.

Here ComputeDistinctiveDescriptors picks the next entry of a fixed per-point table.  Each target keyframe has, per
point p, two features inside p's window: A_p (close to the table's entry 0) and B_p (close to entry 1), so a changed
descriptor changes the best feature."""
import numpy as np

import kf_projection_cases as cases

f32 = np.float32
TH_LOW = 50
NPOINTS, NTARGETS = 30, 4


class MapPoint:
    def __init__(self, mid, table):
        self.id, self.table, self.version = mid, table, 0
        self.desc = table[0]
        self.obs = {}          # KeyFrame -> feature index
        self.bad = False

    def nobs(self):
        return len(self.obs)

    def compute_distinctive_descriptors(self):
        self.version = min(self.version + 1, len(self.table) - 1)
        self.desc = self.table[self.version]

    def replace(self, other, log):                       # MapPoint::Replace
        if other is self:
            return
        obs, self.obs, self.bad = self.obs, {}, True
        for kf, idx in obs.items():
            if kf not in other.obs:
                kf.mp[idx] = other
                other.obs[kf] = idx
            else:
                kf.mp[idx] = None
        before = other.desc
        other.compute_distinctive_descriptors()
        log.append((other.id, bool((before != other.desc).any())))


class KeyFrame:
    def __init__(self, kid, n):
        self.id, self.mp = kid, [None] * n


def build(seed=5):
    """(targets, points): targets = [(kf dict for the searches, pts dict, KeyFrame)], points = the MapPoints whose
    projections pts holds, in order."""
    from oracle import KP_DTYPE
    rng = np.random.default_rng(seed)
    d0 = rng.integers(0, 256, (NPOINTS, 32), dtype=np.uint8)
    d1 = rng.integers(0, 256, (NPOINTS, 32), dtype=np.uint8)
    points = []
    for p in range(NPOINTS):
        v0 = cases._flip(rng, d0[p], 3)
        v1 = cases._flip(rng, d1[p], 3) if p % 2 == 0 else v0          # odd points: the recomputed bytes are the same
        points.append(MapPoint(p, [v0, v1, v1]))
    home = KeyFrame(-1, NPOINTS)                                        # the current keyframe observes every point
    for p, mp in enumerate(points):
        home.mp[p], mp.obs[home] = mp, p
    px = (40 + 25 * (np.arange(NPOINTS) % 10)).astype(f32)
    py = (40 + 25 * (np.arange(NPOINTS) // 10)).astype(f32)
    level = np.ones(NPOINTS, np.int32)
    targets, next_id = [], 1000
    for k in range(NTARGETS):
        n = 2 * NPOINTS
        perm = rng.permutation(n)                                       # feature index of A_p: perm[2p], of B_p: perm[2p+1]
        kps = np.zeros(n, KP_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        for p in range(NPOINTS):
            a, b = perm[2 * p], perm[2 * p + 1]
            kps["x"][a], kps["y"][a], desc[a] = px[p], py[p], d0[p]
            kps["x"][b], kps["y"][b], desc[b] = px[p] + 1, py[p], d1[p]
        kps["octave"] = 1
        kf = dict(desc=desc, kps=kps, bounds=cases.BOUNDS, uright=np.full(n, -1, f32), inv_sigma2=cases.INV_SIGMA2)
        pts = dict(u=(px + f32(0.5)).astype(f32), v=py.copy(), ur=(px - 2).astype(f32), level=level,
                   radius=(cases.TH * cases.SCALE[level]).astype(f32),
                   desc=np.ascontiguousarray(np.stack([mp.table[0] for mp in points])))
        node = KeyFrame(k, n)
        for p in range(NPOINTS):
            kind = (p + 3 * k) % 6
            if kind in (0, 1, 2):                                       # a MapPoint already at A_p (0, 1) or B_p (2)
                e = MapPoint(next_id, [rng.integers(0, 256, 32, dtype=np.uint8)])
                next_id += 1
                idx = perm[2 * p] if kind < 2 else perm[2 * p + 1]
                node.mp[idx], e.obs[node] = e, int(idx)
                if kind == 1:                                           # ... with more observations than the point
                    for j in range(3):
                        ph = KeyFrame(next_id, 1)
                        next_id += 1
                        ph.mp[0], e.obs[ph] = e, 0
        targets.append((kf, pts, node))
    return targets, points


def state(targets, points):
    """The graph as plain data: per target the ids at its features, per point its flag, observations and bytes."""
    return ([[None if m is None else m.id for m in node.mp] for _, _, node in targets],
            [(mp.bad, sorted((kf.id, idx) for kf, idx in mp.obs.items()), mp.desc.tobytes()) for mp in points])


def run(targets, points, search, scw):
    """The caller's loop.  search(k, i, mp) -> (bestIdx, bestDist) of point i in target k.  scw: SearchAndFuse's form
    (Fuse fills vpReplacePoints, the caller replaces afterwards) instead of SearchInNeighbors'.  Returns (nFused per
    target, the Replace log [(survivor id, descriptor changed)], the searches made [(k, i, descriptor version)])."""
    log, asked, nfused_all = [], [], []
    for k, (_, _, node) in enumerate(targets):
        nfused = 0
        replace_points = [None] * len(points)
        for i, mp in enumerate(points):
            if mp.bad or node in mp.obs:                                # :849 / :1005 (spAlreadyFound)
                continue
            asked.append((k, i, mp.version))
            best_idx, best_dist = search(k, i, mp)
            if best_idx >= 0 and best_dist <= TH_LOW:                   # :952 / :1082
                in_kf = node.mp[best_idx]
                if in_kf is not None:
                    if not in_kf.bad:
                        if scw:
                            replace_points[i] = in_kf                   # :1088
                        elif in_kf.nobs() > mp.nobs():                  # :959-962
                            mp.replace(in_kf, log)
                        else:
                            in_kf.replace(mp, log)
                else:
                    mp.obs[node] = best_idx                             # :967-968 / :1092-1093
                    node.mp[best_idx] = mp
                nfused += 1
        if scw:                                                         # LoopClosing.cc:591-612: pRep->Replace(mvpLoopMapPoints[i])
            for i, rep in enumerate(replace_points):
                if rep is not None:
                    rep.replace(points[i], log)
        nfused_all.append(nfused)
    return nfused_all, log, asked


def replay(batch_search, single_search, scw, dirty_rule=True, seed=5):
    """Build the toy, search every (target, point) at once with batch_search(targets) -> per target (best_idx,
    best_dist), then run the loop from those results, taking single_search(target, i, descriptor) for a point whose
    descriptor bytes changed since (unless dirty_rule is off).  Returns (state, nFused, log, asked)."""
    targets, points = build(seed)
    batched = batch_search(targets)
    seen = [mp.desc.copy() for mp in points]

    def search(k, i, mp):
        if dirty_rule and (mp.desc != seen[i]).any():
            return single_search(targets[k], i, mp.desc)
        return int(batched[k][0][i]), int(batched[k][1][i])
    nfused, log, asked = run(targets, points, search, scw)
    return state(targets, points), nfused, log, asked


def sequential(single_search, scw, seed=5):
    """The reference's order of work: every search when its point comes up, with the descriptor it has then."""
    targets, points = build(seed)
    nfused, log, asked = run(targets, points, lambda k, i, mp: single_search(targets[k], i, mp.desc), scw)
    return state(targets, points), nfused, log, asked
