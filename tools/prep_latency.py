#!/usr/bin/env python3
"""Times the fisheye driver's front door on the GPU and prints one JSON line:

  device batch   orb_front_prep_device (k_front_prep) on N BGR frames of the camera's 1920 x 1208 resident on the device,
                 with the reference's camera mask (tests/golden/mask_new_front.npz) and the driver's crop (0, 0, 1900,
                 800).  The yardstick, in the same run and alternating with it round by round: orb_to_gray_device on N
                 BGR frames of 1900 x 800, which reads the same source bytes and writes four times as many.  Every round
                 is `reps` queued calls ending in a synchronise, after warm-up; the JSON carries every round's time, the
                 medians, the yardstick's own spread ((max - min) / median over the rounds) and the ratio.
  host frame     orb_extract_fisheye on one 1920 x 1208 host BGR frame against the CPU chain orb_front_prep_host (mask,
                 crop, resize and gray in one single-thread pass) + orb_extract: `runs` runs of `host_reps` calls each,
                 median and slowest run.

There is no fallback: without a GPU the tool fails.  The outputs are compared before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-birdview_amd"))

SW, SH, CROP = 1920, 1208, (0, 0, 1900, 800)


def _timed(call, sync, reps, warmup):
    for _ in range(warmup):
        call()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    sync()
    return (time.perf_counter() - t0) / reps * 1e3   # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--host-reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prep_latency: no GPU")
    import orbgpu
    from orbgpu import _lib
    from orbgpu.synth import synth_frame
    L = _lib.lib()
    n = a.frames
    cx, cy, cw, ch = CROP
    ow, oh = cw // 2, ch // 2

    g = np.load(os.path.join(ROOT, "tests", "golden", "mask_new_front.npz"))
    keep = np.unpackbits(g["keep_bits"], axis=1)[:, :SW].astype(bool)
    mask = np.where(keep, 0, 255).astype(np.uint8)
    # distinct colour frames: 4 scenes per channel, repeated over the batch
    base = np.stack([np.stack([synth_frame(SW, SH, 3 * i + c) for c in range(3)], -1) for i in range(4)])
    sel = np.arange(n) % len(base)
    out = {"frames": n, "source": [SW, SH], "crop": list(CROP), "reps": a.reps, "rounds": a.rounds}

    ctx = orbgpu._Ctx(2000, 1.2, 8, 15, 5, 0)
    prep = orbgpu.FrontPrep(ctx, (SW, SH), mask, CROP)
    alloc = lambda nbytes: L.orb_device_alloc(ctx.h, nbytes)
    sync = lambda: orbgpu.check(L.orb_sync(ctx.h), "orb_sync")
    fbytes, cbytes = SW * SH * 3, cw * ch * 3
    d_src, d_crop = alloc(n * fbytes), alloc(n * cbytes)
    d_small, d_gray = alloc(n * ow * oh), alloc(n * cw * ch)
    assert d_src and d_crop and d_small and d_gray
    try:
        for f in range(n):
            fr = base[sel[f]]
            orbgpu.check(L.orb_memcpy_h2d(ctx.h, d_src + f * fbytes, fr.ctypes.data, fbytes), "h2d")
            cr = np.ascontiguousarray(fr[cy:cy + ch, cx:cx + cw])
            orbgpu.check(L.orb_memcpy_h2d(ctx.h, d_crop + f * cbytes, cr.ctypes.data, cbytes), "h2d")
        prep_call = lambda: orbgpu.front_prep_device(ctx, prep, orbgpu.COLOR_BGR, d_src, n, fbytes, SW * 3, d_small,
                                                     ow * oh, ow)
        gray_call = lambda: orbgpu.check(L.orb_to_gray_device(ctx.h, orbgpu.COLOR_BGR, d_crop, n, cw, ch, cbytes, cw * 3,
                                                              d_gray, cw * ch, cw), "orb_to_gray_device")
        prep_call()
        sync()
        got = np.zeros((n, oh, ow), np.uint8)
        orbgpu.check(L.orb_memcpy_d2h(ctx.h, got.ctypes.data, d_small, got.nbytes), "d2h")
        want = np.stack([orbgpu.front_prep_host(b, mask, CROP, orbgpu.COLOR_BGR) for b in base])[sel]
        assert np.array_equal(got, want), "device front image differs from the CPU definition"

        prep_ms, gray_ms = [], []
        for _ in range(a.rounds):   # alternating, so that both see the same machine
            gray_ms.append(_timed(gray_call, sync, a.reps, a.warmup))
            prep_ms.append(_timed(prep_call, sync, a.reps, a.warmup))
        pm, gm = statistics.median(prep_ms), statistics.median(gray_ms)
        out["front_prep_ms_rounds"] = prep_ms
        out["to_gray_ms_rounds"] = gray_ms
        out["front_prep_ms"] = pm
        out["to_gray_ms"] = gm
        out["to_gray_spread"] = (max(gray_ms) - min(gray_ms)) / gm
        out["front_prep_spread"] = (max(prep_ms) - min(prep_ms)) / pm
        out["front_prep_over_to_gray"] = pm / gm
        out["front_prep_bytes"] = n * (cbytes + ow * oh + 2 * ((ow + 3) // 4) * oh)
        out["to_gray_bytes"] = n * (cbytes + cw * ch)
        out["front_prep_GBps"] = out["front_prep_bytes"] / pm / 1e6
        out["to_gray_GBps"] = out["to_gray_bytes"] / gm / 1e6
    finally:
        prep.close()
        for p in (d_src, d_crop, d_small, d_gray):
            L.orb_device_free(ctx.h, p)
        ctx.close()

    one = orbgpu.ORBextractor(2000, 1.2, 8, 15, 5)
    prep = orbgpu.FrontPrep(one, (SW, SH), mask, CROP)
    try:
        img = np.ascontiguousarray(base[0])
        k1, d1 = one(img, color=orbgpu.COLOR_BGR, prep=prep)
        k2, d2 = one(orbgpu.front_prep_host(img, mask, CROP, orbgpu.COLOR_BGR))
        assert k1.tobytes() == k2.tobytes() and np.array_equal(d1, d2), "orb_extract_fisheye differs from orb_extract"
        nothing = lambda: None
        gpu_call = lambda: one(img, color=orbgpu.COLOR_BGR, prep=prep)
        cpu_call = lambda: one(orbgpu.front_prep_host(img, mask, CROP, orbgpu.COLOR_BGR))
        gpu_runs, cpu_runs, def_runs = [], [], []
        for _ in range(a.runs):
            gpu_runs.append(_timed(gpu_call, nothing, a.host_reps, 3))
            cpu_runs.append(_timed(cpu_call, nothing, a.host_reps, 3))
            def_runs.append(_timed(lambda: orbgpu.front_prep_host(img, mask, CROP, orbgpu.COLOR_BGR), nothing,
                                   a.host_reps, 3))
        for name, runs in (("extract_fisheye", gpu_runs), ("cpu_prep_plus_extract", cpu_runs), ("cpu_prep", def_runs)):
            out[name + "_ms_median"] = statistics.median(runs)
            out[name + "_ms_slowest"] = max(runs)
        out["keypoints"] = len(k1)
    finally:
        prep.close()
        one.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
