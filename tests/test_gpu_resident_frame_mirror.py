"""GPU: the C++ host mirror's ResidentFrame (host/ORBmatcher.{h,cc}).  tests/cpp_resident_frame/
test_resident_frame_mirror runs one projection case (SearchByProjection(CurrentFrame, LastFrame), stereo, rotation
check) and one Fuse case (chi-square gate) with the train side as FrameGrid plus arrays and as a ResidentFrame; both
forms must give the same vectors, and those of the reference loops."""
import os
import subprocess

import numpy as np
import pytest

import kf_projection_cases as kc
import projection_cases as pc
from test_gpu_projection_mirror import _case_bytes, _f, _i

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_resident_frame")
PROJ, FUSE = "cflf_stereo_th15_ori", 1


def _fuse_bytes(kf, pts, chi2):
    f32, i32 = (lambda a: np.asarray(a, np.float32).tobytes()), (lambda a: np.asarray(a, np.int32).tobytes())
    nt = len(kf["kps"])
    return b"".join([_i(nt), np.ascontiguousarray(kf["kps"]).tobytes(), np.ascontiguousarray(kf["desc"]).tobytes(),
                     _f(*kf["bounds"]), f32(kf["uright"]), _i(len(kf["inv_sigma2"])), f32(kf["inv_sigma2"]), _i(int(chi2)),
                     _i(len(pts["u"])), f32(pts["u"]), f32(pts["v"]), f32(pts["ur"]), f32(pts["radius"]),
                     i32(pts["level"]), np.ascontiguousarray(pts["desc"], np.uint8).tobytes()])


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_resident_frame_mirror")


@pytest.mark.gpu
def test_resident_frame_overloads_equal_the_frame_grid_overloads(mirror_bin, oracle_mod, tmp_path):
    kf, pts = kc.fuse_targets()[FUSE]
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(_case_bytes(pc.case(PROJ)) + _fuse_bytes(kf, pts, True))
    p = subprocess.run([mirror_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = np.frombuffer(dst.read_bytes(), np.int32)
    want_m, want_n, _ = pc.expected(oracle_mod, PROJ)
    n_grid, n_res, nt = (int(x) for x in res[:3])
    m_grid, m_res = res[3:3 + nt], res[3 + nt:3 + 2 * nt]
    assert nt == len(want_m) and n_grid == n_res == want_n
    assert np.array_equal(m_grid, want_m) and np.array_equal(m_res, want_m)
    o = 3 + 2 * nt
    nq = int(res[o])
    best = res[o + 1:o + 1 + 4 * nq].reshape(2, nq, 2)
    want_i, want_d, _ = kc.expected_fuse(oracle_mod, FUSE, True)
    assert nq == len(want_i) and (want_i >= 0).sum() > 20
    for b in best:
        assert np.array_equal(b[:, 0], want_i) and np.array_equal(b[:, 1], want_d)
    assert res[o + 1 + 4 * nq] == 1, "the resident frame's grid differs from FrameGrid's"
    assert len(res) == o + 2 + 4 * nq
