#!/usr/bin/env python3
"""Per-call time of the grid searches with the train side as host pointers (staged and uploaded on every call) and as a
resident orb_frame handle, on one MI355X, for the same inputs: orb_search_by_projection (the CF/LF form, th 15, stereo)
against orb_search_by_projection_frame, and a 10-target orb_project_best_batch (gate FUSE) against
orb_project_best_frames, at 640x480 / 1,000 and 1,280x720 / 2,000; and orb_frame_create itself.  Host wall time around
the synchronous C call (arguments marshalled once).  Each form is timed in ROUNDS rounds of CALLS calls after WARMUP
warm-up calls, the two forms taking turns, so the spread of a form's round medians (max - min) is the run-to-run
spread the difference is read against.

    python profiles/time_resident_frame.py > profiles/time_resident_frame.txt
"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_projection import f32, orbgpu, p, workload, _lib  # noqa: E402

WARMUP, CALLS, ROUNDS = 20, 200, 3


def rounds(fns):
    """{name: fn} -> {name: per-round medians in us}, the forms taking turns."""
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            for _ in range(WARMUP):
                fn()
            t = []
            for _ in range(CALLS):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            out[k].append(statistics.median(t))
    return out


def row(size, call, form, med):
    return dict(size=size, call=call, form=form, median_us=round(statistics.median(med), 1),
                round_medians_us=[round(x, 1) for x in med], spread_us=round(max(med) - min(med), 1))


def main():
    L = _lib.lib()
    rows = []
    for w, h, nf in [(640, 480, 1000), (1280, 720, 2000)]:
        W = workload(w, h, nf)
        m = W["m"]
        ctx = m._ctx.h
        inv_w, inv_h, off, idx = W["grid"]
        g = _lib.OrbFrameGrid(0.0, 0.0, inv_w, inv_h, off.ctypes.data, idx.ctypes.data)
        nt, q = len(W["kb"]), W["cflf"]
        size = f"{w}x{h} nq={len(q)} nt={nt}"
        out_h, out_r, nm = np.zeros(nt, np.int32), np.zeros(nt, np.int32), ctypes.c_int()
        F = orbgpu.Frame(m, W["db"], W["kb"], bounds=(0, w, 0, h), uright=W["uright"])

        def host():
            st = L.orb_search_by_projection(ctx, 0, 0.8, 1, 100, len(q), p(q), p(W["da"]), nt, p(W["db"]), p(W["kb"]),
                                            p(W["uright"]), None, g, p(out_h), ctypes.byref(nm))
            assert st == 0, st

        def resident():
            st = L.orb_search_by_projection_frame(ctx, 0, 0.8, 1, 100, len(q), p(q), p(W["da"]), F.h, None, 1, p(out_r),
                                                  ctypes.byref(nm))
            assert st == 0, st

        r = rounds({"host pointers": host, "resident": resident})
        assert np.array_equal(out_h, out_r)
        for k, med in r.items():
            rows.append(row(size, "search_by_projection CF/LF th15 stereo", k, med))

        # Fuse: 10 targets, each this frame with a tenth of the points
        inv_s2 = (f32(1) / (f32(1.2) ** (2 * np.arange(8)))).astype(f32)
        fq = W["fmp"].copy()
        fq["min_level"], fq["max_level"] = -1, -1
        parts = np.array_split(np.arange(len(fq)), 10)
        keep, th, tr = [], (_lib.OrbProjTarget * 10)(), (_lib.OrbProjFrameTarget * 10)()
        for k, sel in enumerate(parts):
            a = [np.ascontiguousarray(fq[sel]), np.ascontiguousarray(W["da"][sel])] + [np.zeros(len(sel), np.int32) for _ in range(4)]
            keep.append(a)
            th[k] = _lib.OrbProjTarget(len(sel), p(a[0]), p(a[1]), nt, p(W["db"]), p(W["kb"]), p(W["uright"]), p(inv_s2), 8,
                                       g, p(a[2]), p(a[3]))
            tr[k] = _lib.OrbProjFrameTarget(len(sel), p(a[0]), p(a[1]), F.h, p(inv_s2), 8, p(a[4]), p(a[5]))

        def fuse_host():
            assert L.orb_project_best_batch(ctx, 1, 10, ctypes.addressof(th)) == 0

        def fuse_res():
            assert L.orb_project_best_frames(ctx, 1, 10, ctypes.addressof(tr)) == 0

        r = rounds({"host pointers": fuse_host, "resident": fuse_res})
        for a in keep:
            assert np.array_equal(a[2], a[4]) and np.array_equal(a[3], a[5])
        for k, med in r.items():
            rows.append(row(size, "project_best FUSE 10 targets", k, med))

        def create():
            h = ctypes.c_void_p()
            st = L.orb_frame_create(ctx, nt, p(W["db"]), p(W["kb"]), p(W["uright"]), 0.0, 0.0, inv_w, inv_h,
                                    ctypes.byref(h))
            assert st == 0, st
            L.orb_frame_destroy(h)

        r = rounds({"create + destroy": create})
        rows.append(row(size, "orb_frame_create", "create + destroy", r["create + destroy"]))
        F.close()
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
