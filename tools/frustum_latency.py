#!/usr/bin/env python3
"""Latency of the searches over resident map points against the staged path of the same work (tools/frustum_latency.cc
has the two paths): orb_search_local_points for 1,000, 3,000 and 10,000 points and orb_fuse_search_points for 10 and 20
targets of 2,000 points each, at 640x480 / 1,000 features and at 1280x720 / 2,000 features.  Median microseconds per
call from the host clock around the synchronous calls, warm-up first; the two paths alternate within one process.

    python3 tools/frustum_latency.py [--reps 200] [--out profiles/frustum_latency.json]

The binary is built from tools/frustum_latency.cc against the in-tree liborbgpu.so when it is missing or older than
its source."""
import argparse
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
SRC = os.path.join(ROOT, "tools", "frustum_latency.cc")
EXE = os.path.join(ROOT, "tools", "frustum_latency")
FRAMES = ((640, 480, 1000), (1280, 720, 2000))
LOCAL_POINTS = (1000, 3000, 10000)
FUSE_TARGETS, FUSE_POINTS = (10, 20), 2000


def build():
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= os.path.getmtime(SRC):
        return
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC, "-L" + PKG, "-lorbgpu",
                           "-Wl,-rpath,$ORIGIN/../orb-slam-birdview_amd"])


def run(*args):
    p = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (args, p.stdout[-500:], p.stderr[-2000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build()
    rows = []
    for w, h, nf in FRAMES:
        for n in LOCAL_POINTS:
            rows.append(run(w, h, nf, "local", n, a.reps))
        for nt in FUSE_TARGETS:
            rows.append(run(w, h, nf, "fuse", nt, FUSE_POINTS, a.reps))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
