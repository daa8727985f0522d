#!/usr/bin/env python3
"""Times the colour front door on the GPU and prints one JSON line:

  device batch   orb_to_gray_device on N BGR frames of W x H resident on the device, its bytes moved ((3 + 1) W H N)
                 and GB/s; in the same run a plain device-to-device copy moving the same total bytes (2 W H N bytes
                 read and as many written: the yardstick), and orb_extract_batch_device on the same batch for
                 proportion.  Times are a host clock around `reps` queued calls ending in a synchronise, after warm-up.
  host frame     orb_extract_color on one W x H host BGR frame against orb_to_gray_host (the single-thread CPU loop of
                 the same formula) + orb_extract.

There is no fallback: without a GPU the tool fails.  The outputs are compared before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-birdview_amd"))


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
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=200)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gray_latency: no GPU")
    import orbgpu
    from orbgpu import _lib
    from orbgpu.synth import synth_frame
    L = _lib.lib()
    n, w, h = a.frames, a.width, a.height

    # distinct colour frames: 8 scenes per channel, repeated over the batch
    base = np.stack([np.stack([synth_frame(w, h, 3 * i + c) for c in range(3)], -1) for i in range(8)])
    bgr = base[np.arange(n) % 8]
    ext = orbgpu.BatchExtractor(a.nfeatures, w, h, n)
    out = {"frames": n, "width": w, "height": h, "nfeatures": a.nfeatures, "reps": a.reps}
    try:
        ext.upload_color(bgr, orbgpu.COLOR_BGR)
        ext.sync()
        got = np.zeros((n, h, w), np.uint8)
        orbgpu.check(L.orb_memcpy_d2h(ext.h, got.ctypes.data, ext.d_frames, got.nbytes), "d2h")
        want = np.stack([orbgpu.to_gray_host(base[i], orbgpu.COLOR_BGR) for i in range(8)])[np.arange(n) % 8]
        assert np.array_equal(got, want), "device gray differs from the CPU definition"

        gray_call = lambda: orbgpu.check(L.orb_to_gray_device(ext.h, orbgpu.COLOR_BGR, ext.d_color, n, w, h, w * h * 3,
                                                              w * 3, ext.d_frames, w * h, w), "orb_to_gray_device")
        ms = _timed(gray_call, ext.sync, a.reps, a.warmup)
        moved = 4 * w * h * n
        out["to_gray_ms"] = ms
        out["to_gray_bytes"] = moved
        out["to_gray_GBps"] = moved / ms / 1e6

        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda").random_(0, 256)
        dst = torch.empty_like(src)
        cms = _timed(lambda: dst.copy_(src), torch.cuda.synchronize, a.reps, a.warmup)
        out["copy_ms"] = cms
        out["copy_bytes"] = moved
        out["copy_GBps"] = moved / cms / 1e6
        out["to_gray_over_copy"] = ms / cms
        del src, dst

        out["extract_batch_ms"] = _timed(ext.launch, ext.sync, max(a.reps // 5, 3), 2)
        out["to_gray_plus_extract_ms"] = _timed(lambda: (gray_call(), ext.launch()), ext.sync, max(a.reps // 5, 3), 2)
    finally:
        ext.close()

    one = orbgpu.ORBextractor(a.nfeatures, 1.2, 8, 20, 7)
    try:
        img = np.ascontiguousarray(base[0])
        k1, d1 = one(img, color=orbgpu.COLOR_BGR)
        k2, d2 = one(orbgpu.to_gray_host(img, orbgpu.COLOR_BGR))
        assert k1.tobytes() == k2.tobytes() and np.array_equal(d1, d2), "orb_extract_color differs from orb_extract"
        nothing = lambda: None
        out["extract_color_ms"] = _timed(lambda: one(img, color=orbgpu.COLOR_BGR), nothing, a.host_reps, 10)
        out["cpu_gray_plus_extract_ms"] = _timed(lambda: one(orbgpu.to_gray_host(img, orbgpu.COLOR_BGR)), nothing,
                                                 a.host_reps, 10)
        out["cpu_gray_ms"] = _timed(lambda: orbgpu.to_gray_host(img, orbgpu.COLOR_BGR), nothing, a.host_reps, 10)
        gray = orbgpu.to_gray_host(img, orbgpu.COLOR_BGR)
        out["extract_gray_ms"] = _timed(lambda: one(gray), nothing, a.host_reps, 10)
    finally:
        one.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
