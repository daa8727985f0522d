"""CPU: the list-decision rule of the matcher replays (csrc/topk_scan.h), without a GPU and without liborbgpu.

tests/cpp_topk_scan/topk_scan_test.cc runs topk_scan on hand-written K = 8 lists: which entries of a ranked list a
replay takes as the reference's best and second best, and when the list cannot decide them, so that the replay ranks
again.  The GPU parity of the replays that use it is tests/test_gpu_matcher.py, test_gpu_projection*.py and
test_gpu_match_bird*.py."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp_topk_scan", "topk_scan_test.cc")


def test_topk_scan_cases(tmp_path):
    exe = str(tmp_path / "topk_scan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
