#!/usr/bin/env python3
"""Times the stereo front door on the GPU and prints one JSON line:

  device batch   orb_remap_device on N raw frames of W x H resident on the device, interleaved left / right through two
                 maps; its bytes (per pixel and frame: 6 map bytes as the kernel loads them, 1 source byte, 1
                 destination byte; the maps are shared by the frames and come from cache, so the bytes from memory are
                 nearer 2 per pixel: both rates are given) and, in the same run, a plain device-to-device copy writing
                 the same destination bytes (the yardstick), and orb_extract_batch_device on the same batch for
                 proportion.  Times are a host clock around `reps` queued calls ending in a synchronise, after warm-up.
  host frame     orb_extract_rectified on one W x H raw host frame against orb_remap_host (the single-thread CPU loop
                 of the same definition) + orb_extract.

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


def _rig(orbgpu, w, h):
    """The maps of a mildly distorted stereo rig of a w x h camera (a 752-wide calibration scaled)."""
    s = w / 752.0
    K = [460.0 * s, 0.0, 368.5 * s, 0.0, 458.25 * s, 249.0 * s * (h / (480.0 * s)), 0.0, 0.0, 1.0]
    P = [436.0 * s, 0.0, 366.25 * s, 0.0, 436.0 * s, 251.5 * s * (h / (480.0 * s)), 0.0, 0.0, 1.0]
    c, sn = np.cos(0.007), np.sin(0.007)
    Rl = [1.0, 0.0, 0.0, 0.0, c, -sn, 0.0, sn, c]
    Rr = [1.0, 0.0, 0.0, 0.0, c, sn, 0.0, -sn, c]
    return (orbgpu.rectify_maps_host(K, [-0.28, 0.074, 0.0002, 1.8e-05, 0.0], Rl, P, (w, h)),
            orbgpu.rectify_maps_host(K, [-0.27, 0.07, -0.0001, 2.5e-05], Rr, P, (w, h)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=100)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("remap_latency: no GPU")
    import orbgpu
    from orbgpu.synth import synth_frame
    L = orbgpu._lib.lib()
    n, w, h = a.frames, a.width, a.height

    maps = _rig(orbgpu, w, h)
    base = np.stack([synth_frame(w, h, i) for i in range(8)])       # 8 distinct scenes, repeated over the batch
    raw = base[np.arange(n) % 8]
    ext = orbgpu.BatchExtractor(a.nfeatures, w, h, n)
    rects = [orbgpu.Rectifier(ext, mx, my) for mx, my in maps]
    out = {"frames": n, "width": w, "height": h, "nfeatures": a.nfeatures, "reps": a.reps, "map_bytes_per_pixel": 6}
    try:
        ext.upload_raw(raw, rects)
        ext.sync()
        got = np.zeros((n, h, w), np.uint8)
        orbgpu.check(L.orb_memcpy_d2h(ext.h, got.ctypes.data, ext.d_frames, got.nbytes), "d2h")
        for f in range(16):                                          # every scene through both maps
            assert np.array_equal(got[f], orbgpu.remap_host(raw[f], *maps[f % 2])), "device remap differs from the CPU definition"
        assert np.array_equal(got[16:32], got[:16])

        remap_call = lambda: orbgpu.remap_device(ext, rects, ext.d_raw, n, w, h, w * h, w, ext.d_frames, w * h, w)
        ms = _timed(remap_call, ext.sync, a.reps, a.warmup)
        px = w * h * n
        out["remap_ms"] = ms
        out["remap_bytes_counted"] = 8 * px                          # map + source + destination, as loaded and stored
        out["remap_counted_GBps"] = 8 * px / ms / 1e6
        out["remap_image_bytes"] = 2 * px                            # source + destination: what has to come from memory
        out["remap_image_GBps"] = 2 * px / ms / 1e6

        src = torch.empty(px, dtype=torch.uint8, device="cuda").random_(0, 256)
        dst = torch.empty_like(src)
        cms = _timed(lambda: dst.copy_(src), torch.cuda.synchronize, a.reps, a.warmup)
        out["copy_ms"] = cms
        out["copy_bytes"] = 2 * px
        out["copy_GBps"] = 2 * px / cms / 1e6
        out["remap_over_copy"] = ms / cms
        del src, dst

        out["extract_batch_ms"] = _timed(ext.launch, ext.sync, max(a.reps // 5, 3), 2)
        out["remap_plus_extract_ms"] = _timed(lambda: (remap_call(), ext.launch()), ext.sync, max(a.reps // 5, 3), 2)
    finally:
        for r in rects:
            r.close()
        ext.close()

    one = orbgpu.ORBextractor(a.nfeatures, 1.2, 8, 20, 7)
    rect = orbgpu.Rectifier(one, *maps[0])
    try:
        img = np.ascontiguousarray(base[0])
        k1, d1 = one(img, rectify=rect)
        k2, d2 = one(orbgpu.remap_host(img, *maps[0]))
        assert k1.tobytes() == k2.tobytes() and np.array_equal(d1, d2), "orb_extract_rectified differs from orb_extract"
        nothing = lambda: None
        out["extract_rectified_ms"] = _timed(lambda: one(img, rectify=rect), nothing, a.host_reps, 10)
        out["cpu_remap_plus_extract_ms"] = _timed(lambda: one(orbgpu.remap_host(img, *maps[0])), nothing, a.host_reps, 10)
        out["cpu_remap_ms"] = _timed(lambda: orbgpu.remap_host(img, *maps[0]), nothing, a.host_reps, 10)
        rectified = orbgpu.remap_host(img, *maps[0])
        out["extract_gray_ms"] = _timed(lambda: one(rectified), nothing, a.host_reps, 10)
    finally:
        rect.close()
        one.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
