#!/usr/bin/env python3
"""Per-call time of orb_project_best_batch on one MI355X: 1, 10 and 30 target keyframes in one call, at 640x480 /
1,000 trains / 300 projected points per target and at 1280x720 / 2,000 / 800, with and without Fuse's reprojection gate.
Next to it orb_search_by_projection (mode BEST, no rotation check, no stereo gate) on one target of the same shape: the
existing per-keyframe call a caller's loop over N keyframes would make N times.  Host wall time around the
synchronous C call (arguments marshalled once), median of 200 calls after 20 warm-up calls; the kernel's own time
from the context's ORB_K_HAMMING markers in a separate pass.

    python profiles/time_fuse.py > profiles/time_fuse.txt
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


def keyframes(w, h, nf, npts, count):
    """`count` keyframes (views of one synthetic scene shifted by a few pixels) and, per keyframe, npts map points:
    the first view's features projected into it with +-1.5 px of noise at the feature's level or one above."""
    ext = orbgpu.ORBextractor(nf, 1.2, 8, 20, 7)
    scale = np.asarray(ext.GetScaleFactors(), f32)
    inv_sigma2 = np.asarray(ext.GetInverseScaleSigmaSquares(), f32)
    base = synth_frame(w, h, 40)
    k0, d0 = ext(base)
    rng = np.random.default_rng(1)
    out = []
    for j in range(count):
        dx, dy = 1 + j % 7, 1 + j % 5
        kb, db = ext(np.roll(base, (dy, dx), axis=(0, 1)))
        kb, db = np.ascontiguousarray(kb[:nf]), np.ascontiguousarray(db[:nf])
        sel = rng.choice(len(k0), npts, replace=False)
        u = (k0["x"][sel] + dx + rng.uniform(-1.5, 1.5, npts)).astype(f32)
        v = (k0["y"][sel] + dy + rng.uniform(-1.5, 1.5, npts)).astype(f32)
        level = np.minimum(k0["octave"][sel] + rng.integers(0, 2, npts), 7).astype(np.int32)
        uright = np.full(len(kb), -1, f32)
        uright[::3] = np.maximum(kb["x"][::3] - rng.uniform(0.5, 4, len(kb[::3])).astype(f32), 0.0)
        q = orbgpu.proj_queries(u, v, f32(3.0) * scale[level], level, ur=u - f32(2.0))
        out.append(dict(q=q, qdesc=np.ascontiguousarray(d0[sel]), tdesc=db, kps_t=kb,
                        grid=orbgpu.frame_grid(kb, 0, w, 0, h), t_uright=uright, inv_sigma2=inv_sigma2))
    return out


def main():
    L = _lib.lib()
    m = orbgpu.ORBmatcher(0.8, False)
    ctx = m._ctx.h
    rows = []
    for w, h, nf, npts in [(640, 480, 1000, 300), (1280, 720, 2000, 800)]:
        kfs = keyframes(w, h, nf, npts, 30)
        t0 = kfs[0]
        inv_w, inv_h, off, idx = t0["grid"]
        g = _lib.OrbFrameGrid(0.0, 0.0, inv_w, inv_h, off.ctypes.data, idx.ctypes.data)
        nt = len(t0["kps_t"])
        size = f"{w}x{h} nt={nt} npts={npts}"
        out, nm = np.zeros(nt, np.int32), ctypes.c_int()

        def single():
            st = L.orb_search_by_projection(ctx, 0, 0.8, 0, 50, npts, p(t0["q"]), p(t0["qdesc"]), nt, p(t0["tdesc"]),
                                            p(t0["kps_t"]), None, None, g, p(out), ctypes.byref(nm))
            assert st == 0, st
        one = timed(single, ctx)
        rows.append(dict(size=size, call="orb_search_by_projection BEST, one target", targets=1, nmatches=nm.value, **one))
        for gate, name in ((0, "none"), (1, "fuse")):
            for n in (1, 10, 30):
                T = orbgpu._ProjTargets(kfs[:n])

                def batch():
                    st = L.orb_project_best_batch(ctx, gate, n, ctypes.addressof(T.arr))
                    assert st == 0, st
                r = timed(batch, ctx)
                accepted = int(sum(((bi >= 0) & (bd <= 50)).sum() for bi, bd in T.out))
                rows.append(dict(size=size, call=f"orb_project_best_batch gate {name}", targets=n, accepted_th_low=accepted,
                                 n_single_calls_us=round(n * one["median_us"], 1),
                                 ratio_batch_over_n_single=round(r["median_us"] / (n * one["median_us"]), 3), **r))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
