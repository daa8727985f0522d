"""CPU: csrc/grid_window.h (the cell rectangle and candidate filter the grid kernels run) against a transcription of
Frame::GetFeaturesInArea, on windows off and across every side of the grid, on cell boundaries, at r = 0, at exactly
distance r and under the level ranges.  tests/cpp_grid_window/grid_window_test.cc is a stand-alone program, built here
with ASan + UBSan and run directly."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_grid_window_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "grid_window_test")
    src = os.path.join(ROOT, "tests", "cpp_grid_window", "grid_window_test.cc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "grid_window OK" in r.stdout, r.stdout + r.stderr
