"""Pin of the float form of Fuse's reprojection gate, checked on the CPU: tools/fuse_flags_probe.cpp
(ORBmatcher.cc:914-938 written plainly), compiled with the reference's flags, agrees with the explicit fmaf forms that
k_projection_best, orb_project_best_host and tests/kf_projection_ref.py use (tools/fuse_flags_check.cpp, built
-ffp-contract=off), and the test-side exact float32 fmaf agrees with the probe too."""
import json
import os
import subprocess

import numpy as np

import kf_projection_ref as ref
from test_trig_pin import TOOLS, _build, _toolchain, needs_fma


def _f(h):
    return np.array([int(h, 16)], np.uint32).view(np.float32)[0]


@needs_fma
def test_fuse_gate_contraction_forms(tmp_path):
    # -march=x86-64-v3 stands for the reference's -march=native on an AVX2+FMA host (CMakeLists.txt:10-11)
    print("pin scope:", _toolchain())
    exe = _build(str(tmp_path), "chk", [
        ["g++", "-O3", "-march=x86-64-v3", "-std=c++11", "-c", os.path.join(TOOLS, "fuse_flags_probe.cpp"), "-o", "probe.o"],
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-c", os.path.join(TOOLS, "fuse_flags_check.cpp"), "-o", "check.o"],
        ["g++", "-o", "chk", "check.o", "probe.o", "-lm"]])
    out = json.loads(subprocess.check_output([exe, "1000000"], timeout=600))
    print(out)
    assert out["cases"] == 1_000_000 and out["stereo_cases"] > 100_000 and out["skipped"] > 100_000
    assert out["e2_mismatch"] == 0 and out["skip_mismatch"] == 0
    assert out["e2_uncontracted_differs"] > 0          # the contraction is real (e2's last bit)
    # the restatement's exact float32 fmaf against the probe's e2 and verdict
    lines = subprocess.check_output([exe, "dump", "3000"], timeout=600).decode().split("\n")
    n = 0
    for line in lines:
        if not line:
            continue
        w = line.split()
        u, v, ur, kpx, kpy, kpr, inv, e2 = (_f(h) for h in w[:8])
        got, _ = ref.fuse_e2(u, v, ur, kpx, kpy, kpr)
        assert got.tobytes() == e2.tobytes(), line
        assert ref.fuse_gate_skips(u, v, ur, kpx, kpy, kpr, inv)[0] == (w[8] == "1"), line
        n += 1
    assert n == 3000
