"""GPU: the C++ host mirror's three projection-gated searches (host/ORBmatcher.{h,cc}) against
tests/projection_ref.py.  tests/cpp_projection/test_projection_mirror reads the cases this test writes, runs
ORBmatcher::SearchByProjection (both forms) and SearchByProjectionBird, and writes its result vectors back."""
import os
import subprocess

import numpy as np
import pytest

import projection_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_projection")

NAMES = ["cflf_mono_th7_ori", "cflf_stereo_th15_ori", "cflf_forward_th7_ori", "cflf_backward_th15", "fmp_th1", "fmp_th5",
         "fmp_th3_image_bounds", "bird_r10", "exhaustion_best", "exhaustion_ratio", "lanes"]
FORM = {"cflf": 0, "fmp": 1, "bird": 2}


def _i(*v):
    return np.array(v, np.int32).tobytes()


def _f(*v):
    return np.array(v, np.float32).tobytes()


def _case_bytes(c):
    f, p = c["frame"], c["pts"]
    nt = len(f["kps"])
    ur = f.get("uright")
    taken = np.zeros(nt, np.uint8) if f.get("taken") is None else np.asarray(f["taken"], np.uint8)
    out = [_i(FORM[c["form"]], nt), np.ascontiguousarray(f["kps"]).tobytes(), np.ascontiguousarray(f["desc"]).tobytes(),
           _f(*f["bounds"]), _i(0 if ur is None else 1), b"" if ur is None else np.asarray(ur, np.float32).tobytes(),
           taken.tobytes(), np.asarray(f.get("scale_factors", pc.SCALE), np.float32).tobytes(), _f(f.get("mbf", 0.0)),
           _f(c["nnratio"]), _i(int(c.get("check_ori", True))), _f(c["th"] if "th" in c else c["r"]),
           _i(int(c.get("b_mono", False)), int(c.get("forward", False)), int(c.get("backward", False))),
           _i(len(p["desc"]))]
    a32, i32, u8 = (lambda a: np.asarray(a, np.float32).tobytes()), (lambda a: np.asarray(a, np.int32).tobytes()), \
        (lambda a: np.asarray(a, np.uint8).tobytes())
    if c["form"] == "cflf":
        out += [a32(p["u"]), a32(p["v"]), a32(p["invzc"]), i32(p["octave"]), a32(p["angle"]), u8(p["observed"])]
    elif c["form"] == "fmp":
        out += [a32(p["proj_x"]), a32(p["proj_y"]), a32(p["proj_xr"]), i32(p["level"]), a32(p["view_cos"])]
    else:
        out += [a32(p["x"]), a32(p["y"])]
    out.append(np.ascontiguousarray(p["desc"], np.uint8).tobytes())
    return b"".join(out)


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_projection_mirror")


@pytest.mark.gpu
def test_mirror_projection_searches_match_reference(mirror_bin, oracle_mod, tmp_path):
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(_i(len(NAMES)) + b"".join(_case_bytes(pc.case(n)) for n in NAMES))
    p = subprocess.run([mirror_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = np.frombuffer(dst.read_bytes(), np.int32)
    o = 0
    for name in NAMES:
        want_m, want_n, _ = pc.expected(oracle_mod, name)
        n, nt = int(res[o]), int(res[o + 1])
        m = res[o + 2:o + 2 + nt]
        o += 2 + nt
        assert nt == len(want_m) and n == want_n and np.array_equal(m, want_m), (name, n, want_n)
    assert o == len(res)
