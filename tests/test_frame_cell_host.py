"""CPU: csrc/frame_cell.h (the cell arithmetic k_frame_grid runs) on its rounding edges and on values no int holds,
and a host model of the kernel's count / scan / scatter / order algorithm against the reference's push-back loop.
tests/cpp_frame_cell/frame_cell_test.cc is a stand-alone program, built here with ASan + UBSan and run directly."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_frame_cell_and_grid_model_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "frame_cell_test")
    src = os.path.join(ROOT, "tests", "cpp_frame_cell", "frame_cell_test.cc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "frame_cell OK" in r.stdout, r.stdout + r.stderr
