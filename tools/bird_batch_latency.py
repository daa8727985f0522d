#!/usr/bin/env python3
"""Per-frame latency of the birdview stream: B single calls against one batch call (GPU only).

Device-resident 1280x720 frames (orbgpu.synth.bench_frames), one shared mask, BirdORB(2000), warmed up at every
shape.  For B in {1, 4, 16, 64}, five repetitions, A and B alternating in this process:
  A: a loop of B orb_bird_extract_device calls;
  B: one orb_bird_extract_batch_device call.
Wall clock around calls that end in the call's own synchronise; every repetition runs for at least --min-seconds
(default 0.25 s, so every point has more than one second of work).  A sweep of the post-selection group size
at B = 16 and 64 comes first; the table uses the library's default group.  Writes profiles/bird_batch.json.

    python3 tools/bird_batch_latency.py [--out profiles/bird_batch.json]
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

W, H, NF, CAP = 1280, 720, 2000, 2304
BATCHES = (1, 4, 16, 64)
GROUPS = (1, 2, 4, 8, 16, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bird_batch.json"))
    ap.add_argument("--min-seconds", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bird_batch_latency: no GPU")
    import orbgpu
    from orbgpu import KP_DTYPE
    from orbgpu._lib import lib
    from orbgpu.synth import bench_frames, synth_bird_mask

    nmax = max(BATCHES)
    d_imgs = torch.from_numpy(bench_frames(W, H, nmax)).cuda()
    d_mask = torch.from_numpy(synth_bird_mask(W, H, 0)).cuda()
    torch.cuda.synchronize()
    bird = orbgpu.BirdORB(NF)
    L = lib()
    vp = ctypes.c_void_p
    kps_a = np.zeros((nmax, CAP), KP_DTYPE)
    desc_a = np.zeros((nmax, CAP, 32), np.uint8)
    cnt_a = np.zeros(nmax, np.int32)
    kps_b, desc_b, cnt_b = np.zeros_like(kps_a), np.zeros_like(desc_a), np.zeros_like(cnt_a)
    img0, mask0, fp = d_imgs.data_ptr(), d_mask.data_ptr(), W * H
    ka, da, ca = kps_a.ctypes.data, desc_a.ctypes.data, cnt_a.ctypes.data
    pk, pd, pc = vp(kps_b.ctypes.data), vp(desc_b.ctypes.data), vp(cnt_b.ctypes.data)

    def run_a(B):
        for f in range(B):
            st = L.orb_bird_extract_device(bird.h, vp(img0 + f * fp), W, H, W, vp(mask0), W,
                                           vp(ka + f * CAP * KP_DTYPE.itemsize), CAP,
                                           ctypes.cast(ca + 4 * f, ctypes.POINTER(ctypes.c_int)), vp(da + f * CAP * 32))
            assert st == 0, st

    def run_b(B):
        st = L.orb_bird_extract_batch_device(bird.h, B, vp(img0), W, H, W, fp, vp(mask0), W, 0, pk, pd, CAP, pc)
        assert st == 0, st

    def per_frame_us(fn, B):
        """calls of fn(B) until min-seconds have passed -> microseconds per frame"""
        n, t0 = 0, time.perf_counter()
        while True:
            fn(B)
            n += 1
            dt = time.perf_counter() - t0
            if dt >= args.min_seconds:
                return dt / (n * B) * 1e6

    def stats(v):
        return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                "spread_us": round(max(v) - min(v), 2), "reps_us": [round(x, 2) for x in v]}

    default_group = bird.batch_group()
    for B in BATCHES:   # warm-up at every shape (buffers grow to the largest batch)
        run_b(B)
        run_a(B)
    run_b(nmax)
    equal = all(cnt_a[f] == cnt_b[f] and kps_a[f, :cnt_a[f]].tobytes() == kps_b[f, :cnt_b[f]].tobytes() and
                desc_a[f, :cnt_a[f]].tobytes() == desc_b[f, :cnt_b[f]].tobytes() for f in range(nmax))

    sweep = {}
    for B in (16, 64):
        sweep[str(B)] = {}
        for g in GROUPS:
            if g > B:
                continue
            bird.batch_group(g)
            run_b(B)
            sweep[str(B)][str(g)] = round(min(per_frame_us(run_b, B) for _ in range(3)), 2)
    bird.batch_group(default_group)

    table = {}
    for B in BATCHES:
        a, b = [], []
        for _ in range(args.reps):
            a.append(per_frame_us(run_a, B))
            b.append(per_frame_us(run_b, B))
        table[str(B)] = {"single_calls": stats(a), "batch_call": stats(b)}
        print(f"B={B:3d}  A {statistics.median(a):8.2f} us/frame (spread {max(a) - min(a):.2f})   "
              f"B {statistics.median(b):8.2f} us/frame (spread {max(b) - min(b):.2f})", flush=True)
    r16 = table["16"]
    result = {
        "tool": "tools/bird_batch_latency.py", "device": torch.cuda.get_device_name(0), "width": W, "height": H,
        "nfeatures": NF, "mask": "shared", "min_seconds_per_rep": args.min_seconds, "reps": args.reps,
        "group_size": default_group, "group_sweep_us_per_frame": sweep, "per_frame_us": table,
        "keypoints_per_frame_mean": float(cnt_b[:nmax].mean()), "outputs_equal": bool(equal),
        "purpose_met_at_16": bool(r16["single_calls"]["median_us"] - r16["batch_call"]["median_us"] >
                                  r16["single_calls"]["spread_us"]),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"group_size": default_group, "sweep": sweep, "outputs_equal": equal,
                      "purpose_met_at_16": result["purpose_met_at_16"]}))
    bird.close()
    if not equal:
        sys.exit("bird_batch_latency: the batch call's outputs differ from the single calls'")


if __name__ == "__main__":
    main()
