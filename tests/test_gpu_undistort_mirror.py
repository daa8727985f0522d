"""The host mirror (C++) and the Python binding of the undistort step give the C-ABI's results: UndistortKeyPoints and
ComputeImageBounds equal the host twin, and the ResidentFrame factories over extraction slots (FromExtraction,
FromBatch) build the grids of orb_frame_create over the host-twin-undistorted keypoints.  The C++ side runs as
tests/cpp_undistort/test_undistort_mirror on a case written here."""
import os
import struct
import subprocess

import numpy as np
import pytest

import undistort_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_undistort")
W, H, CAP = 320, 240, 200
COUNTS = np.array([150, 200, 0, 65], np.int32)
NCELL = 64 * 48 + 1


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_undistort_mirror")


def _case(orbgpu, cal):
    rng = np.random.default_rng(17)
    nf = len(COUNTS)
    k = np.zeros(nf * CAP, orbgpu.KP_DTYPE)
    k.view(np.uint8).reshape(-1, 28)[:] = rng.integers(0, 256, (nf * CAP, 28), dtype=np.uint8)
    p = ref.seeded_points(cal, W, H, nf * CAP, 23)
    k["x"], k["y"] = p[:, 0], p[:, 1]
    k["octave"] = rng.integers(0, 8, nf * CAP)
    desc = rng.integers(0, 256, (nf * CAP, 32), dtype=np.uint8)
    return k, desc


def _read_frame(buf, pos):
    n = struct.unpack_from("<i", buf, pos)[0]
    off = np.frombuffer(buf, np.int32, NCELL, pos + 4)
    ns = struct.unpack_from("<i", buf, pos + 4 + 4 * NCELL)[0]
    idx = np.frombuffer(buf, np.int32, ns, pos + 8 + 4 * NCELL)
    return (n, off, idx), pos + 8 + 4 * NCELL + 4 * ns


@pytest.mark.parametrize("name", ["yaml", "identity"])
def test_cpp_and_python_mirrors(orbgpu_mod, mirror_bin, tmp_path, name):
    cal = ref.YAML if name == "yaml" else (350.0, 351.0, 160.0, 120.0, (0.0, 1.0, 1.0, 1.0))
    k, desc = _case(orbgpu_mod, cal)
    c32 = ref.calib32(cal)
    src, dst = tmp_path / "case.bin", tmp_path / "results.bin"
    with open(src, "wb") as f:
        f.write(np.array(c32[:4] + c32[4], f32).tobytes())
        f.write(np.array([W, H, len(COUNTS), CAP], np.int32).tobytes())
        f.write(COUNTS.tobytes() + k.tobytes() + desc.tobytes())
    p = subprocess.run([mirror_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    buf = dst.read_bytes()

    # what the C-ABI gives: the host twin's keypoints and bounds, orb_frame_create's grids over them
    d = orbgpu_mod.distortion(*cal)
    bounds = orbgpu_mod.image_bounds(d, W, H)
    un = orbgpu_mod.undistort_points_host(d, np.stack([k["x"], k["y"]], 1))
    k_un = k.copy()
    k_un["x"], k_un["y"] = un[:, 0], un[:, 1]
    m = orbgpu_mod.ORBmatcher(0.8, True)

    def grid_of(f):
        s = slice(f * CAP, f * CAP + COUNTS[f])
        F = orbgpu_mod.Frame(m, desc[s], k_un[s], bounds=tuple(bounds))
        try:
            return (len(F),) + F.grid()
        finally:
            F.close()

    def same(got, want):
        return got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])

    # C++
    assert buf[:16] == bounds.tobytes()
    n0 = struct.unpack_from("<i", buf, 16)[0]
    assert n0 == COUNTS[0] and buf[20:20 + 28 * n0] == k_un[:n0].tobytes()
    pos = 20 + 28 * n0
    one, pos = _read_frame(buf, pos)
    assert same(one, grid_of(1))
    for f in range(len(COUNTS)):
        got, pos = _read_frame(buf, pos)
        assert same(got, grid_of(f)), f
    assert pos == len(buf)

    # Python
    got, _ = orbgpu_mod.undistort_keypoints(m, d, k[:COUNTS[0]])
    assert got.tobytes() == k_un[:COUNTS[0]].tobytes()
    assert orbgpu_mod.image_bounds(d, W, H).tobytes() == ref.image_bounds(cal, W, H).tobytes()
