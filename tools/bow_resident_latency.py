#!/usr/bin/env python3
"""Times the vocabulary-gated searches between resident frames against their host-pointer forms, in
one process on the same data, and prints one JSON line.  Shapes as profiles/time_projection.py: C2 = 1,000 features,
C3 = 2,000.  Every figure is the median of `reps` synchronous calls after `warmup` calls, in microseconds; the C entry
points are called directly with arguments built once, so neither form pays for Python conversions.

  tri_1 / tri_10      SearchForTriangulation, one neighbour and ten per call
  bow_kf_f_1 / _10    SearchByBoW(KF, F), one keyframe and ten per call
  bow_kf_kf           SearchByBoW(KF, KF)
  compute_bow_1 / _64 orb_frame_compute_bow on 1 and 64 handles against orb_vocab_transform + orb_vocab_bow per frame

The data: random descriptors; the second view is the first with 12 random bits flipped per descriptor and the
keypoints moved 6 px to the right, so the searches find matches; a synthetic k = 10, L = 3 vocabulary with levelsup 1
(100 FeatureVector nodes, ORBvoc's count at levelsup 4 of 6).  The outputs of both forms are compared before anything
is timed.  There is no fallback: without a GPU the tool fails."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-birdview_amd"))


def _median_us(call, reps, warmup):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return statistics.median(t) * 1e6


def _views(orbgpu, n, seed):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    flip = np.zeros((n, 256), np.uint8)
    for i in range(n):
        flip[i, rng.choice(256, 12, replace=False)] = 1
    d2 = d1 ^ np.packbits(flip, axis=1)
    k1 = np.zeros(n, orbgpu.KP_DTYPE)
    k1["x"], k1["y"] = rng.uniform(20, 1260, n), rng.uniform(20, 700, n)
    k1["angle"], k1["octave"] = rng.uniform(0, 360, n), rng.integers(0, 8, n)
    k2 = k1.copy()
    k2["x"] += 6.0
    ur = [np.where(rng.random(n) < 0.5, k["x"] - 10.0, -1.0).astype(np.float32) for k in (k1, k2)]
    mp = [(rng.random(n) < 0.4).astype(np.uint8) for _ in range(2)]
    return (d1, k1, ur[0], mp[0]), (d2, k2, ur[1], mp[1])


def _shape(orbgpu, L, m, voc, n, reps, warmup):
    from orbgpu import _lib
    ci, p = ctypes.c_int, lambda a: ctypes.c_void_p(a.ctypes.data)
    (d1, k1, ur1, mp1), (d2, k2, ur2, mp2) = _views(orbgpu, n, n)
    b = (0.0, 1280.0, 0.0, 720.0)
    F1, F2 = orbgpu.Frame(m, d1, k1, bounds=b, uright=ur1), orbgpu.Frame(m, d2, k2, bounds=b, uright=ur2)
    out = {}
    try:
        orbgpu.compute_bow(voc, [F1, F2], 1)
        fvs = [F.bow(voc)[1] for F in (F1, F2)]
        assert fvs[0] == voc.transform(d1, 1)[1]
        fv1, keep1 = orbgpu._featvec(fvs[0])
        fv2, keep2 = orbgpu._featvec(fvs[1])
        F12 = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)
        lv = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
        s2 = (lv * lv).astype(np.float32)
        no_mp = [np.zeros(n, np.uint8), np.zeros(n, np.uint8)]   # a new keyframe pair: nothing triangulated yet
        a1, a2 = np.ascontiguousarray(k1["angle"]), np.ascontiguousarray(k2["angle"])
        h = m._ctx.h
        for nn in (1, 10):
            cap = n + 1
            ho = [np.zeros((cap, 2), np.int32) for _ in range(nn)]
            ro = [np.zeros((cap, 2), np.int32) for _ in range(nn)]
            hc, rc = [ci() for _ in range(nn)], [ci() for _ in range(nn)]
            HP = (_lib.OrbTriPair * nn)(*[_lib.OrbTriPair(n, p(d2), p(k2), p(no_mp[1]), p(ur2), fv2, p(F12), -1000.0, 360.0,
                                                          p(lv), p(s2), 8, p(ho[i]), cap, ctypes.pointer(hc[i]))
                                          for i in range(nn)])
            RP = (_lib.OrbTriFramePair * nn)(*[_lib.OrbTriFramePair(F2.h, p(no_mp[1]), p(F12), -1000.0, 360.0, p(lv), p(s2), 8,
                                                                    p(ro[i]), cap, ctypes.pointer(rc[i]))
                                               for i in range(nn)])
            host = lambda: L.orb_search_for_triangulation_batch(h, 0, 0, n, p(d1), p(k1), p(no_mp[0]), p(ur1), fv1, nn,
                                                                ctypes.cast(HP, ctypes.c_void_p))
            res = lambda: L.orb_search_for_triangulation_frames(h, 0, 0, F1.h, p(no_mp[0]), nn, ctypes.cast(RP, ctypes.c_void_p))
            assert host() == 0 and res() == 0
            for i in range(nn):
                assert hc[i].value == rc[i].value > 0 and np.array_equal(ho[i], ro[i])
            out[f"tri_{nn}"] = {"host_us": _median_us(host, reps, warmup), "resident_us": _median_us(res, reps, warmup),
                                "pairs": hc[0].value}
            ho = [np.full(n, -1, np.int32) for _ in range(nn)]
            ro = [np.full(n, -1, np.int32) for _ in range(nn)]
            HK = (_lib.OrbBowKf * nn)(*[_lib.OrbBowKf(n, p(d1), p(a1), p(mp1), fv1, p(ho[i]), ctypes.pointer(hc[i]))
                                        for i in range(nn)])
            RK = (_lib.OrbBowFrameKf * nn)(*[_lib.OrbBowFrameKf(F1.h, p(mp1), p(ro[i]), ctypes.pointer(rc[i]))
                                             for i in range(nn)])
            host = lambda: L.orb_search_by_bow_kf_f_batch(h, 0.7, 1, n, p(d2), p(a2), fv2, nn, ctypes.cast(HK, ctypes.c_void_p))
            res = lambda: L.orb_search_by_bow_frames_kf_f(h, 0.7, 1, F2.h, nn, ctypes.cast(RK, ctypes.c_void_p))
            assert host() == 0 and res() == 0
            for i in range(nn):
                assert hc[i].value == rc[i].value > 0 and np.array_equal(ho[i], ro[i])
            out[f"bow_kf_f_{nn}"] = {"host_us": _median_us(host, reps, warmup),
                                     "resident_us": _median_us(res, reps, warmup), "matches": hc[0].value}
        ho, ro, hc, rc = np.full(n, -1, np.int32), np.full(n, -1, np.int32), ci(), ci()
        host = lambda: L.orb_search_by_bow_kf_kf(h, 0.7, 1, n, p(d1), p(a1), p(mp1), fv1, n, p(d2), p(a2), p(mp2), fv2, p(ho),
                                                 ctypes.byref(hc))
        res = lambda: L.orb_search_by_bow_frames_kf_kf(h, 0.7, 1, F1.h, p(mp1), F2.h, p(mp2), p(ro), ctypes.byref(rc))
        assert host() == 0 and res() == 0 and hc.value == rc.value > 0 and np.array_equal(ho, ro)
        out["bow_kf_kf"] = {"host_us": _median_us(host, reps, warmup), "resident_us": _median_us(res, reps, warmup),
                            "matches": hc.value}
        # ComputeBoW: the handles' form against transform + bow per frame through the host arrays
        frames = [orbgpu.Frame(m, d1, k1, bounds=b) for _ in range(64)]
        try:
            w, wt, nd = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
            bw, bv, fn, fo, fi = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.uint32), np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
            nb, nf = ci(), ci()
            vh = voc._ctx.h

            def host_one():
                assert L.orb_vocab_transform(vh, voc.v, p(d1), n, 1, p(w), p(wt), p(nd)) == 0
                assert L.orb_vocab_bow(voc.v, n, p(w), p(wt), p(nd), p(bw), p(bv), ctypes.byref(nb), p(fn), p(fo), p(fi),
                                       ctypes.byref(nf)) == 0

            for cnt in (1, 64):
                hs = (ctypes.c_void_p * cnt)(*[f.h for f in frames[:cnt]])
                res = lambda: L.orb_frame_compute_bow(vh, voc.v, 1, cnt, hs)
                host = lambda: [host_one() for _ in range(cnt)]
                assert res() == 0
                out[f"compute_bow_{cnt}"] = {"host_us": _median_us(host, max(reps // (1 if cnt == 1 else 10), 5), 2),
                                             "resident_us": _median_us(res, max(reps // (1 if cnt == 1 else 10), 5), 2)}
            assert frames[63].bow(voc)[1] == fvs[0]
        finally:
            for f in frames:
                f.close()
    finally:
        F1.close()
        F2.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bow_resident_latency: no GPU")
    import orbgpu
    from orbgpu.synth import write_synth_vocab
    L = orbgpu._lib.lib()
    m = orbgpu.ORBmatcher(0.7, True)
    voc = orbgpu.ORBVocabulary()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "voc.bin")
        write_synth_vocab(path, 10, 3, seed=1)
        voc.loadFromBinaryFile(path)
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "us, median"}
    try:
        for name, n in (("C2", 1000), ("C3", 2000)):
            out[name] = _shape(orbgpu, L, m, voc, n, a.reps, a.warmup)
    finally:
        voc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
