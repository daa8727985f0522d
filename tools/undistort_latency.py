#!/usr/bin/env python3
"""Latency of making a resident frame from an extraction's raw output slot: orb_frame_create_from_extract (undistort
and grid on the GPU) and orb_frames_create_from_batch at 8 frames, against the only route there was before them:
keypoints and descriptors to the host, orb_undistort_points_host as the CPU loop, then orb_frame_create.  1,000,
2,000 and 4,000 keypoints per frame, spread over 640x480 and 1280x720, the reference's fisheye calibration scaled to
the image.  Median microseconds per call from the host clock around the synchronous calls (through ctypes: about a
microsecond per call on either side), warm-up first; the routes alternate within one process.  Destroying the handles
is outside the timed span on both sides.

    python3 tools/undistort_latency.py [--reps 200] [--out profiles/undistort_latency.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-birdview_amd"))
FRAMES = ((640, 480), (1280, 720))
COUNTS = (1000, 2000, 4000)
BATCH = 8
K = (-0.0488316, 0.000298406, -0.00591118, 0.00193258)   # Examples/Monocular/fisheye.yaml


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import orbgpu
    from orbgpu import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    m = orbgpu.ORBmatcher(0.8, True)
    h = m._ctx.h
    rows = []
    for w, hgt in FRAMES:
        s = w / 950.0
        dist = orbgpu.distortion(348.5 * s, 347.0 * s, 480.0 * s, 302.0 * s, K)
        b = orbgpu.image_bounds(dist, w, hgt)
        inv_w = float(np.float32(64) / (b[1] - b[0]))
        inv_h = float(np.float32(48) / (b[3] - b[2]))
        grid = (float(b[0]), float(b[2]), inv_w, inv_h)
        for n in COUNTS:
            rng = np.random.default_rng(n)
            k = np.zeros(BATCH * n, orbgpu.KP_DTYPE)
            k["x"], k["y"] = rng.uniform(16, w - 16, len(k)), rng.uniform(16, hgt - 16, len(k))
            k["octave"] = rng.integers(0, 8, len(k))
            desc = rng.integers(0, 256, (len(k), 32), dtype=np.uint8)
            counts = np.full(BATCH, n, np.int32)
            d_k, d_d, d_c = (L.orb_device_alloc(h, x.nbytes) for x in (k, desc, counts))
            for p, x in ((d_k, k), (d_d, desc), (d_c, counts)):
                _lib.check(L.orb_memcpy_h2d(h, p, vp(x.ctypes.data), x.nbytes), "h2d")
            hk, hd = np.zeros(n, orbgpu.KP_DTYPE), np.zeros((n, 32), np.uint8)
            xy, un = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
            out1, out8 = vp(), (vp * BATCH)()

            def resident(f=0):
                _lib.check(L.orb_frame_create_from_extract(h, ctypes.byref(dist), n, vp(d_d + f * n * 32),
                                                           vp(d_k + f * n * 28), None, *grid, ctypes.byref(out1)), "new")
                return [out1.value]

            def staged(f=0):
                _lib.check(L.orb_memcpy_d2h(h, vp(hk.ctypes.data), vp(d_k + f * n * 28), hk.nbytes), "d2h")
                _lib.check(L.orb_memcpy_d2h(h, vp(hd.ctypes.data), vp(d_d + f * n * 32), hd.nbytes), "d2h")
                xy[:, 0], xy[:, 1] = hk["x"], hk["y"]
                _lib.check(L.orb_undistort_points_host(ctypes.byref(dist), n, vp(xy.ctypes.data), vp(un.ctypes.data)),
                           "host")
                hk["x"], hk["y"] = un[:, 0], un[:, 1]
                _lib.check(L.orb_frame_create(h, n, vp(hd.ctypes.data), vp(hk.ctypes.data), None, *grid,
                                              ctypes.byref(out1)), "old")
                return [out1.value]

            def resident_batch():
                _lib.check(L.orb_frames_create_from_batch(h, ctypes.byref(dist), BATCH, vp(d_d), vp(d_k), vp(d_c), n,
                                                          *grid, out8), "batch")
                return list(out8)

            def staged_batch():
                return [staged(f)[0] for f in range(BATCH)]

            def clock(fn):
                t0 = time.perf_counter_ns()
                handles = fn()
                t = time.perf_counter_ns() - t0
                for x in handles:
                    L.orb_frame_destroy(vp(x))
                return t / 1000.0

            row = {"width": w, "height": hgt, "keypoints": n, "batch": BATCH, "reps": a.reps}
            for name, new, old in (("single", resident, staged), ("batch", resident_batch, staged_batch)):
                for _ in range(10):
                    clock(new), clock(old)
                t_new, t_old = [], []
                for _ in range(a.reps):
                    t_new.append(clock(new))
                    t_old.append(clock(old))
                row[name + "_resident_us"] = round(statistics.median(t_new), 1)
                row[name + "_staged_us"] = round(statistics.median(t_old), 1)
                row[name + "_ratio"] = round(row[name + "_staged_us"] / row[name + "_resident_us"], 2)
            for p in (d_k, d_d, d_c):
                L.orb_device_free(h, p)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
