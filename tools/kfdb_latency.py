#!/usr/bin/env python3
"""Latency of one keyframe-database query: orb_kfdb_query on the GPU against the reference's inverted-file query on one
CPU thread (tools/kfdb_cpu_query, built by tests/cpp_kfdb/Makefile), at two sizes:

    small   1,000 keyframes x about 500 words over a 10^5-word id space
    large   5,000 keyframes x about 1,000 words over a 10^6-word id space

both with a 1,000-word query, on seeded synthetic L1-normalised vectors.  The GPU figure is the host clock around the
synchronous call (upload of the query, one launch, one synchronisation, the host's sort of the sharing list); the CPU
figure covers the sharing list, the 0.8f cut and the scores of the keyframes above it, which is what the reference
computes; the GPU call scores every keyframe that shares a word.  Warm-up calls first, then --reps timed ones; medians.

    python3 tools/kfdb_latency.py [--reps 200] [--out profiles/kfdb_latency.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-birdview_amd"))
CPU_TOOL = os.path.join(ROOT, "tools", "kfdb_cpu_query")

SIZES = {"small": (1000, 500, 10 ** 5), "large": (5000, 1000, 10 ** 6)}
QUERY_WORDS = 1000


def vector(rng, n, space):
    w = np.unique(rng.integers(0, space, n)).astype(np.int32)    # about n words, ascending
    v = rng.random(len(w)) + 0.01
    return w, v / v.sum()


def build(name):
    nkf, nwords, space = SIZES[name]
    rng = np.random.default_rng(nkf)
    vecs = [vector(rng, nwords, space) for _ in range(nkf)]
    # a query that resembles a keyframe: half of one keyframe's words, the rest drawn like any vector's
    w0 = vecs[nkf // 2][0]
    half = rng.choice(w0, min(len(w0), QUERY_WORDS // 2), replace=False)
    qw = np.unique(np.concatenate([half, rng.integers(0, space, QUERY_WORDS - len(half))])).astype(np.int32)
    qv = rng.random(len(qw)) + 0.01
    return vecs, (qw, qv / qv.sum())


def gpu_times(vecs, query, reps, warmup=20):
    import orbgpu
    L = orbgpu._lib.lib()
    db = orbgpu.KeyFrameDatabase(device=0)
    try:
        for w, v in vecs:
            db.add(w, v)
        qw, qv = query
        cap = len(db)
        ids, com, sc = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        n = ctypes.c_int()
        args = (db._ctx.h, db.h, len(qw), qw.ctypes.data, qv.ctypes.data, 0, None, None, cap, ids.ctypes.data,
                com.ctypes.data, sc.ctypes.data, ctypes.byref(n))
        us = []
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            st = L.orb_kfdb_query(*args)
            t1 = time.perf_counter()
            assert st == 0, L.orb_last_error()
            if r >= warmup:
                us.append((t1 - t0) * 1e6)
        us.sort()
        return {"gpu_query_us_median": round(us[len(us) // 2], 2), "gpu_query_us_min": round(us[0], 2),
                "listed": n.value, "reps": reps}
    finally:
        db.close()


def cpu_times(vecs, query, reps):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vectors.bin")
        with open(path, "wb") as f:
            f.write(np.int32(len(vecs) + 1).tobytes())
            for w, v in vecs + [query]:
                f.write(np.int32(len(w)).tobytes() + w.astype(np.int32).tobytes() + v.astype(np.float64).tobytes())
        out = subprocess.run([CPU_TOOL, path, str(reps)], check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sizes", default="small,large")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {}
    for name in a.sizes.split(","):
        vecs, query = build(name)
        r = {"keyframes": len(vecs), "words_per_keyframe": int(np.mean([len(w) for w, _ in vecs])),
             "query_words": int(len(query[0])), "word_space": SIZES[name][2]}
        r.update(cpu_times(vecs, query, a.reps))
        g = gpu_times(vecs, query, a.reps)
        assert g["listed"] == r["listed"], (g["listed"], r["listed"])    # both list the same keyframes
        r.update(g)
        r["cpu_over_gpu"] = round(r["cpu_query_us_median"] / r["gpu_query_us_median"], 3)
        result[name] = r
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
