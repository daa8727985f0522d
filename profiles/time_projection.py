#!/usr/bin/env python3
"""Per-call time of orb_search_by_projection on one MI355X: the CF/LF form (SearchByProjection(CurrentFrame,
LastFrame), th 15, stereo) and the F/MapPoints form (SearchByProjection(F, MapPoints), th 3) at two sizes, each with
both lane mappings of k_projection_topk (ORBGPU_PROJ_LANES = 16: a query per 16-lane row; 64: a query per wavefront),
and orb_window_match_grid (SearchForInitialization's shape, window 100) at the same sizes as the yardstick from existing
code with the same staging pattern.  Host wall time around the synchronous C call (arguments marshalled once), median
of 200 calls after 20 warm-up calls; the kernel's own time from the context's ORB_K_HAMMING markers in a separate pass.

    python profiles/time_projection.py > profiles/time_projection.txt
"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-birdview_amd"))
import orbgpu  # noqa: E402
from orbgpu import _lib  # noqa: E402
from orbgpu.synth import synth_frame  # noqa: E402

WARMUP, CALLS = 20, 200
f32 = np.float32


def p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def timed(fn, ctx):
    L = _lib.lib()
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    L.orb_profile_enable(ctx, 1)
    for _ in range(50):
        fn()
    ms, n = np.zeros(7, np.float64), np.zeros(7, np.int32)
    L.orb_profile_read(ctx, p(ms), p(n))
    L.orb_profile_enable(ctx, 0)
    t.sort()
    return dict(median_us=round(statistics.median(t), 1), p10_us=round(t[len(t) // 10], 1),
                p90_us=round(t[9 * len(t) // 10], 1), kernel_us=round(1e3 * ms[4] / max(n[4], 1), 1),
                launches_per_call=round(n[4] / 50, 2))


def workload(w, h, nf):
    a = synth_frame(w, h, 40)
    b = np.roll(a, (3, 5), axis=(0, 1))
    ext = orbgpu.ORBextractor(nf, 1.2, 8, 20, 7)
    ka, da = ext(a)
    kb, db = ext(b)
    ka, da = ka[:nf], np.ascontiguousarray(da[:nf])          # nf queries
    rng = np.random.default_rng(1)
    scale = ext.GetScaleFactors()
    n = len(ka)
    u = (ka["x"] + 5 + rng.uniform(-2, 2, n)).astype(f32)
    v = (ka["y"] + 3 + rng.uniform(-2, 2, n)).astype(f32)
    uright = np.full(len(kb), -1, f32)
    uright[::3] = np.maximum(kb["x"][::3] - rng.uniform(0.5, 4, len(kb[::3])).astype(f32), 0.5)
    grid = orbgpu.frame_grid(kb, 0, w, 0, h)
    m = orbgpu.ORBmatcher(0.8, True)
    cflf = np.zeros(n, orbgpu.PROJ_QUERY_DTYPE)
    cflf["u"], cflf["v"], cflf["r"] = u, v, f32(15) * scale[ka["octave"]]
    cflf["min_level"], cflf["max_level"] = ka["octave"] - 1, ka["octave"] + 1
    cflf["ur"], cflf["ur_tol"] = u - f32(40) * rng.uniform(0.01, 0.1, n).astype(f32), cflf["r"]
    cflf["angle"], cflf["blocks"] = ka["angle"], rng.random(n) >= 0.2
    fmp = np.zeros(n, orbgpu.PROJ_QUERY_DTYPE)
    fmp["u"], fmp["v"] = u, v
    fmp["r"] = np.where(rng.random(n) < 0.5, f32(2.5), f32(4.0)).astype(f32) * f32(3) * scale[ka["octave"]]
    fmp["min_level"], fmp["max_level"] = ka["octave"] - 1, ka["octave"]
    fmp["ur"], fmp["ur_tol"], fmp["blocks"] = u - f32(2), fmp["r"], 1
    return dict(m=m, ka=ka, da=da, kb=np.ascontiguousarray(kb), db=np.ascontiguousarray(db), uright=uright, grid=grid,
                cflf=cflf, fmp=fmp, w=w, h=h)


def candidates(W, q):
    """Candidates per query before the taken / stereo gates (what the reference's inner loop visits)."""
    return [len(orbgpu.features_in_area(W["kb"], 0, W["w"], 0, W["h"], float(x["u"]), float(x["v"]), float(x["r"]),
                                        int(x["min_level"]), int(x["max_level"]))) for x in q]


def main():
    L = _lib.lib()
    rows = []
    for w, h, nf in [(640, 480, 1000), (1280, 720, 2000)]:
        W = workload(w, h, nf)
        ctx = W["m"]._ctx.h
        inv_w, inv_h, off, idx = W["grid"]
        g = _lib.OrbFrameGrid(0.0, 0.0, inv_w, inv_h, off.ctypes.data, idx.ctypes.data)
        nt = len(W["kb"])
        out, nm = np.zeros(max(nt, len(W["ka"])), np.int32), ctypes.c_int()
        size = f"{w}x{h} nq={len(W['ka'])} nt={nt}"
        for form, mode, q, ori in [("CF/LF th15 stereo", 0, W["cflf"], 1), ("F/MapPoints th3", 1, W["fmp"], 0)]:
            cand = candidates(W, q)
            res = {}
            for lanes in (16, 64):
                os.environ["ORBGPU_PROJ_LANES"] = str(lanes)

                def call():
                    st = L.orb_search_by_projection(ctx, mode, 0.8, ori, 100, len(q), p(q), p(W["da"]), nt, p(W["db"]),
                                                    p(W["kb"]), p(W["uright"]), None, g, p(out), ctypes.byref(nm))
                    assert st == 0, st
                res[lanes] = (timed(call, ctx), nm.value, out[:nt].copy())
            assert res[16][1] == res[64][1] and np.array_equal(res[16][2], res[64][2]), "lane mappings disagree"
            for lanes in (16, 64):
                rows.append(dict(size=size, call=f"orb_search_by_projection {form}", lanes=lanes, nmatches=res[lanes][1],
                                 candidates_total=int(sum(cand)), candidates_mean=round(float(np.mean(cand)), 1),
                                 candidates_max=int(max(cand)), **res[lanes][0]))
        os.environ.pop("ORBGPU_PROJ_LANES", None)

        def yard():
            st = L.orb_window_match_grid(ctx, 0.9, 1, 1, len(W["ka"]), p(W["da"]), p(W["ka"]), None, 100.0, nt, p(W["db"]),
                                         p(W["kb"]), g, p(out), ctypes.byref(nm))
            assert st == 0, st
        rows.append(dict(size=size, call="orb_window_match_grid level0 window 100", lanes=64, nmatches=None,
                         **timed(yard, ctx)))
        rows[-1]["nmatches"] = nm.value
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
