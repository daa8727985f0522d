"""Named, deterministic inputs that put every decision of both SearchByBoW forms (ORBmatcher.cc:159-288, :522-655) at
its edge.  Pure numpy; tests/test_bow_cases.py checks on the CPU that tests/bow_ref.py and the oracle agree on every
case and that every planted decision is realised in the reference trace; tests/test_gpu_bow_cases.py runs the same
arrays through k_topk and the host replay (csrc/matcher.hip), one call per case and stacked as a batch.

Side 1 is the keyframe whose features are visited (the queries); side 2 is the Frame (kf_f form) or the second
keyframe (kf_kf form): the same arrays serve both forms, and a Plant states the expected outcome under each.
Descriptors are planted: a partner at Hamming distance d is a descriptor with exactly d chosen bit positions flipped,
and a filler is 256 random bits (about 128 from everything; the cases assert more than 80).  All edge nodes use angle
0 on both sides, so every accepted match falls into rotation bin 0 and the histogram culls nothing; the rotation
edges have cases of their own (rot_*), one single-candidate pair per node with planted angles.

A case is built once and never modified."""
import collections
import functools

import numpy as np

import bow_ref as ref
from planted_tools import ROT_TIED, ROT_TIED_EXPECTED, Builder, Rot, sizes as _sizes

Case = collections.namedtuple("Case", "name nnratio desc1 angle1 mp1 fv1 desc2 angle2 mp2 fv2 plants rot fillers")
# exp_kf_f / exp_kf_kf: (outcome, bestDist1, bestDist2, best index on side 2); None = not pinned
Plant = collections.namedtuple("Plant", "item idx1 exp_kf_f exp_kf_kf")

ITEMS = (
    "th_low_49", "th_low_50", "th_low_51", "ratio_equal", "ratio_below", "ratio_float_0p6_30_50",
    "second_best_ties_best_across_lanes", "one_candidate", "kf_map_point_missing_or_bad",
    "train_map_point_missing_or_bad", "taken_within_node", "taken_across_nodes", "no_common_node",
    "lower_bound_skip_side1", "lower_bound_skip_side2", "lower_bound_skips_two_nodes", "lower_bound_runs_off_the_end",
    "decoy_in_another_node", "node_above_64_candidates", "node_above_512_candidates", "best_beyond_lane_stride",
    "topk_list_exhausted_by_taken",
    "rot_negative_wrap", "rot_bin_30_to_0", "rot_round_half", "maxima_first_second_tied", "maxima_third_tied_first_wins",
    "maxima_third_at_cutoff_kept", "maxima_third_below_cutoff", "maxima_second_below_cutoff",
)


class _B(Builder):
    Plant = Plant

    def done(self, rot=None):
        a = lambda x, t: np.ascontiguousarray(np.array(x, t))
        c = Case(self.name, self.nnratio, a(self.d[0], np.uint8).reshape(-1, 32), a(self.ang[0], np.float32),
                 a(self.mp[0], np.uint8), {k: list(v) for k, v in self.fv[0].items()},
                 a(self.d[1], np.uint8).reshape(-1, 32), a(self.ang[1], np.float32), a(self.mp[1], np.uint8),
                 {k: list(v) for k, v in self.fv[1].items()}, tuple(self.plants), rot, tuple(self.fillers))
        for x in (c.desc1, c.angle1, c.mp1, c.desc2, c.angle2, c.mp2):
            x.setflags(write=False)
        return c


A, D, R, N = ref.ACCEPTED, ref.DIST, ref.RATIO, ref.NO_MP


def _edges():
    b = _B("edges", 11, 0.5)
    # node 5 on side 1 only, node 6 on side 2 only: the walk jumps side 1 with lower_bound, then side 2; node 5's
    # query has its exact copy under node 6, which must not be found
    q = b.rand()
    i = b.add(1, 5, q)
    b.add(2, 6, q.copy())
    b.plants.append(Plant("decoy_in_another_node", i, None, None))
    b.plants.append(Plant("lower_bound_skip_side1", i, None, None))
    b.plants.append(Plant("lower_bound_skip_side2", i, None, None))
    b.simple("th_low_50", 10, (50, 200), (A, 50, 200, 0), (D, 50, 200, 0))       # <= TH_LOW (:228), < TH_LOW (:598)
    b.simple("th_low_51", 11, (51, 200), (D, 51, 200, 0))
    b.simple("th_low_49", 12, (49, 200), (A, 49, 200, 0))
    b.simple("ratio_equal", 13, (20, 40), (R, 20, 40, 0))                       # 20 < 0.5f * 40 is false
    b.simple("ratio_below", 14, (19, 40), (A, 19, 40, 0))
    # a second best that ties the best: else if(dist<bestDist2) gives bestDist2 == bestDist1.  The two sit at list
    # positions 2 and 67 of a 70-candidate node: different lanes of the 64-lane stride, more than 64 apart
    q = b.rand()
    i = b.add(1, 15, q)
    b.fill(15, 67)
    t0 = b.add(2, 15, b.flip(q, range(0, 10)), pos=2)
    b.add(2, 15, b.flip(q, range(10, 20)), pos=67)
    b.add(2, 15, b.flip(q, range(20, 110)))
    assert b.fv[1][15].index(t0) == 2 and len(b.fv[1][15]) == 70
    b.plant("second_best_ties_best_across_lanes", i, (R, 10, 10, t0))
    b.plants.append(Plant("node_above_64_candidates", i, None, None))
    b.simple("one_candidate", 16, (40,), (A, 40, 256, 0))
    # a keyframe feature without a (good) MapPoint is not a query, though its exact copy is a candidate
    q = b.rand()
    i = b.add(1, 17, q, mp=0)
    b.add(2, 17, q.copy())
    b.plant("kf_map_point_missing_or_bad", i, (N, None, None, -1))
    # side 2's MapPoint flags count in the kf_kf form only (:576-580)
    q = b.rand()
    i = b.add(1, 18, q)
    t0 = b.add(2, 18, q.copy(), mp=0)
    t1 = b.add(2, 18, b.flip(q, range(0, 15)))
    b.add(2, 18, b.flip(q, range(15, 75)))
    b.plant("train_map_point_missing_or_bad", i, (A, 0, 15, t0), (A, 15, 60, t1))
    # two nodes in a row on side 1 only: one lower_bound passes both
    b.add(1, 25, b.rand())
    b.add(1, 26, b.rand())
    # within one node: qa (first) takes f1, which qb (second) would have liked better
    qb = b.rand()
    f1, f2, f3 = b.flip(qb, range(0, 3)), b.flip(qb, range(10, 30)), b.flip(qb, range(40, 85))
    ia = b.add(1, 27, b.flip(f1, range(100, 105)))
    ib = b.add(1, 27, qb)
    t1, t2, t3 = b.add(2, 27, f3), b.add(2, 27, f2), b.add(2, 27, f1)
    b.plant("taken_within_node", ia, (A, 5, 28, t3))
    b.plant("taken_within_node", ib, (A, 20, 45, t2))
    b.plants.append(Plant("lower_bound_skips_two_nodes", ib, None, None))
    # across nodes: g1 is listed under nodes 28 and 29 on side 2; node 28's query takes it first
    qd = b.rand()
    g1 = b.flip(qd, range(0, 2))
    ic = b.add(1, 28, b.flip(g1, range(100, 104)))
    tg1 = b.add(2, 28, g1)
    b.add(2, 28, b.flip(qd, range(100, 220)))
    idd = b.add(1, 29, qd)
    b.add(2, 29, b.flip(qd, range(50, 94)))
    b.list_again(2, 29, tg1)
    tg3 = b.add(2, 29, b.flip(qd, range(20, 38)))
    b.plant("taken_across_nodes", ic, (A, 4, 118, tg1))
    b.plant("taken_across_nodes", idd, (A, 18, 44, tg3))
    # one node with 600 candidates.  Q's eight nearest (10..17 bits away, at list positions on both sides of the
    # 64-lane stride and at the list's end) are each the exact partner (3 bits) of an earlier query, so when Q's
    # turn comes its top-8 list holds taken candidates only while 592 others remain: the list is ranked again.
    # Q then takes t8 (30) with t9 (62) second: 30 < 0.5f * 62.
    Q = b.rand()
    sizes, at, near = [10 + k for k in range(8)] + [30, 62], 0, []
    for s in sizes:
        near.append(b.flip(Q, range(at, at + s)))
        at += s
    assert at == 200
    b.fill(30, 590)
    for p, t in sorted(zip((5, 70, 130, 200, 300, 400, 511, 599, 64, 63), range(10))):
        near[t] = (b.add(2, 30, near[t], pos=p), near[t])
    assert [b.fv[1][30].index(near[t][0]) for t in range(10)] == [5, 70, 130, 200, 300, 400, 511, 599, 64, 63]
    for k in range(8):
        i = b.add(1, 30, b.flip(near[k][1], range(200 + 3 * k, 203 + 3 * k)))
        if k == 7:
            b.plant("best_beyond_lane_stride", i, (A, 3, 50, near[7][0]))      # t0..t6 are taken by now: t8 at 3 + 17 + 30
    i = b.add(1, 30, Q)
    b.plant("topk_list_exhausted_by_taken", i, (A, 30, 62, near[8][0]))
    b.plants.append(Plant("node_above_512_candidates", i, None, None))
    # the walk ends inside lower_bound: side 1's last node is below side 2's last, which nothing matches
    b.add(1, 40, b.rand())
    j = b.add(1, 41, b.rand())
    b.add(2, 39, b.rand())
    b.add(2, 45, b.rand())
    b.plants.append(Plant("lower_bound_runs_off_the_end", j, None, None))
    return b.done()


def _ratio06():
    """0.6f * 50.0f rounds to 30.000002, so bestDist1 = 30 against bestDist2 = 50 passes the float comparison that
    fails in exact arithmetic."""
    b = _B("ratio06", 12, 0.6)
    b.simple("ratio_float_0p6_30_50", 3, (30, 50), (A, 30, 50, 0))
    b.simple("ratio_float_0p6_30_50", 4, (31, 50), (R, 31, 50, 0))
    return b.done()


def _disjoint():
    b = _B("disjoint", 13, 0.5)
    for node in (1, 3, 5):
        q = b.rand()
        i = b.add(1, node, q)
        b.add(2, node + 1, q.copy())
    b.plants.append(Plant("no_common_node", i, None, None))
    return b.done()


def _rot(name, seed, pairs, rot):
    """One accepted single-candidate pair (distance 5) per node; pairs = (angle1, angle2) in node order."""
    b = _B(name, seed, 0.5)
    for n, (a1, a2) in enumerate(pairs):
        q = b.rand()
        b.add(1, n, q, angle=a1)
        b.add(2, n, b.flip(q, range(0, 5)), angle=a2)
    return b.done(rot)


def _rot_cases():
    tied = ROT_TIED
    yield _rot("rot_tied", 21, tied, ROT_TIED_EXPECTED)
    # 11 in bin 0: 1 < 0.1f * 11 drops the third maximum; bins 5 and 12 are both culled
    yield _rot("rot_third_cut", 22, tied + [(0.0, 0.0)],
               Rot(("maxima_third_below_cutoff",), _sizes({0: 11, 1: 10, 5: 1, 12: 1}), (0, 1, -1), 2))
    # 11, 1, 1: the second maximum is below the cut-off too, and both small bins go
    yield _rot("rot_second_cut", 23, [(0.0, 0.0)] * 11 + [(30.0, 0.0), (150.0, 0.0)],
               Rot(("maxima_second_below_cutoff",), _sizes({0: 11, 1: 1, 5: 1}), (0, -1, -1), 2))


@functools.lru_cache(maxsize=None)
def cases():
    out = [_edges(), _ratio06(), _disjoint(), *_rot_cases()]
    return {c.name: c for c in out}


CASES = ("edges", "ratio06", "disjoint", "rot_tied", "rot_third_cut", "rot_second_cut")


def reversed_lists(c):
    """The case with every candidate list of side 2 reversed (a new Case; the arrays are shared, not copied)."""
    return c._replace(fv2={k: v[::-1] for k, v in c.fv2.items()})


def expected(form, c):
    return ref.search_by_bow(form, c.nnratio, True, c.desc1, c.angle1, c.mp1, c.fv1, c.desc2, c.angle2, c.mp2, c.fv2)


NODE_STRIDE = 1000


def stacked(form, names):
    """The cases as keyframes of one batch call.  kf_f: one Frame that holds every case's side 2 (feature indices
    and node ids moved apart per case) and each case's side 1 as a keyframe; kf_kf: one KF1 that holds every case's
    side 1 and each case's side 2 as a KF2.  Returns (shared, parts) with shared = (desc, angle, mp, fv) and parts a
    list of dicts(desc, angle, mp, featvec, offset, n): the shared side's index range of that case."""
    cs = [cases()[n] for n in names]
    sh = 2 if form == "kf_f" else 1
    get = lambda c, what: getattr(c, f"{what}{sh}")
    oth = lambda c, what: getattr(c, f"{what}{3 - sh}")
    off = np.cumsum([0] + [len(get(c, "desc")) for c in cs])
    fv = {}
    parts = []
    for k, c in enumerate(cs):
        for node, lst in get(c, "fv").items():
            fv[node + k * NODE_STRIDE] = [i + int(off[k]) for i in lst]
        parts.append(dict(desc=oth(c, "desc"), angle=oth(c, "angle"), mp=oth(c, "mp"),
                          featvec={node + k * NODE_STRIDE: lst for node, lst in oth(c, "fv").items()},
                          offset=int(off[k]), n=len(get(c, "desc"))))
    shared = (np.concatenate([get(c, "desc") for c in cs]), np.concatenate([get(c, "angle") for c in cs]),
              np.concatenate([get(c, "mp") for c in cs]), fv)
    return shared, parts
