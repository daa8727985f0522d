"""CPU: the launch geometry and index arithmetic of k_resize_rows (the batch path's pyramid resize), without a GPU.

tests/cpp_resize_rows/resize_rows_model.cc takes the library's own coefficient tables and rr_geometry and walks
every block, wave and lane as the kernel does: the block -> tile map is a bijection, every staged chunk and every
LDS read is in bounds, and the strip walk gives the plain two-row formula's value for every pixel.  The GPU parity
of the kernel itself is tests/test_gpu_resize_rows.py."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tests", "cpp_resize_rows", "resize_rows_model.cc")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rr") / "resize_rows_model")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-o", exe, SRC,
                           "-L" + PKG, "-lorbgpu", "-Wl,-rpath," + PKG])
    return exe


def _level(n, scale):
    """ComputePyramid's level size (cvRound: half to even, as Python's round)."""
    return int(round(float(n) / scale))


# (source size, scale): widths one below / at / one above a multiple of the tile width (256) and of 4; heights that
# leave a one-row last strip (h % 8 == 1) and a one-row last tile (h % 32 == 1); the bench's C3 levels
CASES = [(307, 200, 1.2), (306, 39, 1.2), (308, 40, 1.2), (310, 231, 1.2), (1280, 720, 1.2), (1067, 600, 1.2),
         (429, 241, 1.2), (269, 210, 1.05), (270, 35, 1.05), (384, 98, 1.5), (386, 301, 1.5), (300, 200, 1.6),
         (640, 480, 1.9)]


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("sw,sh,scale", CASES)
def test_model_walk_in_bounds_and_exact(model, sw, sh, scale, generic):
    dw, dh = _level(sw, scale), _level(sh, scale)
    out = subprocess.run([model, str(sw), str(sh), str(dw), str(dh), str(generic)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    tiles = int(out.stdout.split()[1])
    assert tiles == -(-dw // 256) * -(-dh // 32)


@pytest.mark.parametrize("sw,sh,scale", [(300, 200, 2.2), (640, 480, 2.5)])
def test_large_scale_factors_are_refused(model, sw, sh, scale):
    """From 2 on a tile spans more source rows than the kernel stages, and a lane's 4 pixels read bytes more than 8 apart:
    rr_geometry leaves the level to the other kernels."""
    dw, dh = _level(sw, scale), _level(sh, scale)
    out = subprocess.run([model, str(sw), str(sh), str(dw), str(dh), "0"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "untiled", (out.stdout, out.stderr)
