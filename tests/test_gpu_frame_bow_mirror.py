"""GPU: the C++ host mirror's BoW on ResidentFrame (host/ORBmatcher.{h,cc}).  tests/cpp_frame_bow/test_frame_bow_mirror
runs the planted "edges" cases of SearchForTriangulation and SearchByBoW through the KeyFrameData overloads and through
the ResidentFrame overloads (SetFeatVec), which must agree with each other and with the references, and compares
ResidentFrame::ComputeBoW / BoW with ORBVocabulary::transform on the same descriptors."""
import os
import subprocess

import numpy as np
import pytest

import bow_cases as bc
import triangulation_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_frame_bow")


def _side(kps, desc, mp, ur, fv):
    i32 = lambda *v: np.asarray(v, np.int32).tobytes()
    out = [i32(len(kps)), np.ascontiguousarray(kps).tobytes(), np.ascontiguousarray(desc, np.uint8).tobytes(),
           np.ascontiguousarray(mp, np.uint8).tobytes(), np.ascontiguousarray(ur, np.float32).tobytes(), i32(len(fv))]
    for node in sorted(fv):
        out += [np.asarray([node], np.uint32).tobytes(), i32(len(fv[node])), i32(*fv[node])]
    return b"".join(out)


def _bow_side(desc, angle, mp, fv):
    k = np.zeros(len(desc), tc.KP_DTYPE)
    k["x"], k["y"], k["angle"] = 100.0, 100.0, angle
    return _side(k, desc, mp, np.full(len(desc), -1.0, np.float32), fv)


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_frame_bow_mirror")


@pytest.mark.gpu
def test_resident_bow_overloads_equal_the_keyframe_data_overloads(mirror_bin, tmp_path):
    from orbgpu.synth import write_synth_vocab
    t, b = tc.cases()["edges"], bc.cases()["edges"]
    f32 = lambda *v: np.asarray(v, np.float32).tobytes()
    src, dst, voc = tmp_path / "cases.bin", tmp_path / "results.bin", tmp_path / "voc.bin"
    write_synth_vocab(str(voc), 10, 3, seed=8)
    src.write_bytes(b"".join([
        _side(t.kps1, t.desc1, t.mp1, t.ur1, t.fv1), _side(t.kps2, t.desc2, t.mp2, t.ur2, t.fv2), f32(*tc.F12.ravel()),
        f32(tc.EX, tc.EY), np.asarray([len(tc.SCALE2)], np.int32).tobytes(), f32(*tc.SCALE2), f32(*tc.SIGMA2),
        f32(b.nnratio), _bow_side(b.desc1, b.angle1, b.mp1, b.fv1), _bow_side(b.desc2, b.angle2, b.mp2, b.fv2)]))
    p = subprocess.run([mirror_bin, str(src), str(voc), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = np.frombuffer(dst.read_bytes(), np.int32)
    assert res[0] == 1
    o = 1
    for only_stereo in (False, True):
        want, _ = tc.expected(t, only_stereo)
        n, same = int(res[o]), int(res[o + 1])
        got = res[o + 2:o + 2 + 2 * n].reshape(n, 2)
        assert same == 1 and n == len(want) and np.array_equal(got, want)
        o += 2 + 2 * n
    assert len(tc.expected(t, False)[0]) > 10
    for form in ("kf_f", "kf_kf"):
        want_n, want, _ = bc.expected(form, b)
        n, same, length = (int(x) for x in res[o:o + 3])
        got = res[o + 3:o + 3 + length]
        assert same == 1 and n == want_n and np.array_equal(got, want)
        o += 3 + length
    assert res[o] == 1, "ResidentFrame::BoW differs from ORBVocabulary::transform"
    assert len(res) == o + 1
