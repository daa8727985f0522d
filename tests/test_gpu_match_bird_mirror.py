"""GPU: the C++ host mirror's two SearchByMatchBird forms (host/ORBmatcher.{h,cc}) against tests/match_bird_ref.py.
tests/cpp_match_bird/test_match_bird_mirror reads the cases this test writes, runs ORBmatcher::SearchByMatchBird
(keyframe and frame form) and writes the vectors the mirror wrote back."""
import os
import subprocess

import numpy as np
import pytest

import match_bird_cases as mc
import match_bird_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_match_bird")

# (the mirror's max_dist is the reference's TH_HIGH: the case with another bound is the C-ABI's)
NAMES = [n for n in sorted(mc.CASES) if mc.case(n).get("max_dist", ref.TH_HIGH) == ref.TH_HIGH]


def _i(*v):
    return np.array(v, np.int32).tobytes()


def _f(*v):
    return np.array(v, np.float32).tobytes()


def _frame_bytes(f):
    return b"".join([_i(len(f["kps"])), np.ascontiguousarray(f["kps"]).tobytes(),
                     np.ascontiguousarray(f["desc"], np.uint8).tobytes(), _f(*f["bounds"])])


def _case_bytes(c):
    if c["form"] == "kf":
        q = c["kf"]
        return b"".join([_i(0), _frame_bytes(c["frame"]), _f(c["nnratio"]), _i(int(c["check_ori"])), _f(c["r"]),
                         _i(len(q["index"])), np.asarray(q["index"], np.int32).tobytes()] +
                        [np.asarray(q[k], np.float32).tobytes() for k in ("x", "y", "angle")] +
                        [np.ascontiguousarray(q["desc"], np.uint8).tobytes()])
    last, mp = c["last"], c["has_mp"]
    return b"".join([_i(1), _frame_bytes(c["cur"]), _f(c["nnratio"]), _i(int(c["check_ori"])), _f(c["window"]),
                     _i(len(last["kps"])), np.ascontiguousarray(last["kps"]).tobytes(),
                     np.ascontiguousarray(last["desc"], np.uint8).tobytes(), _i(0 if mp is None else 1),
                     b"" if mp is None else np.asarray(mp, np.uint8).tobytes()])


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_match_bird_mirror")


@pytest.mark.gpu
def test_mirror_search_by_match_bird_matches_reference(mirror_bin, oracle_mod, tmp_path):
    assert len(NAMES) == len(mc.CASES) - 1 and {mc.case(n)["form"] for n in NAMES} == {"kf", "frame"}
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(_i(len(NAMES)) + b"".join(_case_bytes(mc.case(n)) for n in NAMES))
    p = subprocess.run([mirror_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = np.frombuffer(dst.read_bytes(), np.int32)
    o = 0
    for name in NAMES:
        want_m, want_n, _ = mc.expected(oracle_mod, name)
        n, nt = int(res[o]), int(res[o + 1])
        m = res[o + 2:o + 2 + nt]
        o += 2 + nt
        assert nt == len(want_m) and n == want_n and np.array_equal(m, want_m), (name, n, want_n)
    assert o == len(res)
