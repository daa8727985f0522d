"""GPU: the C++ host mirror's keyframe searches (host/ORBmatcher.{h,cc}) against tests/kf_projection_ref.py.
tests/cpp_kf_projection/test_kf_projection_mirror reads the cases this test writes, runs FuseSearch, FuseSearchOne,
SearchBySim3 and the two keyframe forms of SearchByProjection, and writes its results back."""
import os
import subprocess

import numpy as np
import pytest

import kf_projection_cases as cases
import kf_projection_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_kf_projection")


def _i(*v):
    return np.array(v, np.int32).tobytes()


def _a(a, dt):
    return np.ascontiguousarray(a, dt).tobytes()


def _kf(kf):
    n = len(kf["kps"])
    return b"".join([_i(n), _a(kf["kps"], kf["kps"].dtype), _a(kf["desc"], np.uint8), _a(kf["bounds"], np.float32),
                     _a(kf["uright"], np.float32), _a(kf["inv_sigma2"], np.float32), _a(cases.SCALE, np.float32)])


def _points(p):
    n = len(p["u"])
    ur = p.get("ur", np.zeros(n, np.float32))
    return b"".join([_i(n), _a(p["u"], np.float32), _a(p["v"], np.float32), _a(ur, np.float32),
                     _a(p["radius"], np.float32), _a(p["level"], np.int32), _a(p["desc"], np.uint8)])


def _head(p, n):
    return {k: v[:n] for k, v in p.items()}


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", CPP])   # (build() made it; this only checks that it is up to date)
    return os.path.join(CPP, "test_kf_projection_mirror")


@pytest.mark.gpu
def test_mirror_keyframe_searches_match_reference(mirror_bin, oracle_mod, tmp_path):
    targets = cases.fuse_targets()
    kf1, kf2, p12, p21 = cases.sim3_case()
    lp, lkf, ltaken = cases.loop_case()
    rp, rkf, rtaken, orb_dist, ori = cases.reloc_case()
    blob = [_i(8)]
    for chi2 in (0, 1):
        blob += [_i(chi2, len(targets))] + [_kf(kf) + _points(p) for kf, p in targets]
    sim3 = [(kf1, kf2, p12, p21), (kf2, kf1, p21, p12)]
    for a, b, pa, pb in sim3:
        blob += [_i(2), _kf(a), _kf(b), _points(pa), _a(pa["index"], np.int32), _points(pb), _a(pb["index"], np.int32)]
    loops = [(lp, ltaken), (_head(lp, 150), ~ltaken)]
    for p, taken in loops:
        blob += [_i(3), _kf(lkf), _i(10), _points(p), _a(np.where(taken, 7, -1), np.int32)]
    relocs = [(rp, rtaken, ori), (_head(rp, 150), ~rtaken, False)]
    for p, taken, o in relocs:
        blob += [_i(4), _kf(rkf), _a([10.0], np.float32), _i(orb_dist, int(o)), _points(p), _a(p["angle"], np.float32),
                 _a(taken, np.uint8)]
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    r = subprocess.run([mirror_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = np.frombuffer(dst.read_bytes(), np.int32)
    o = 0

    def take(n):
        nonlocal o
        o += n
        return res[o - n:o].tolist()
    for chi2 in (False, True):
        for k, (kf, p) in enumerate(targets):
            nq = take(1)[0]
            bi, bd, _ = cases.expected_fuse(oracle_mod, k, chi2)
            assert nq == len(bi) and take(nq) == bi.tolist() and take(nq) == bd.tolist(), (chi2, k)
            one = [ref.fuse_one(oracle_mod, kf, p, i, p["desc"][(i + 1) % nq], chi2) for i in range(nq)]
            assert take(nq) == [a for a, _ in one] and take(nq) == [b for _, b in one], (chi2, k)
    for a, b, pa, pb in sim3:
        nfound, vn, _ = ref.search_by_sim3(oracle_mod, a, b, pa, pb)
        assert take(2) == [nfound, len(vn)] and take(len(vn)) == vn.tolist()
    for p, taken in loops:
        match, n, _ = ref.search_kf_scw(oracle_mod, p, lkf, taken)
        assert take(2) == [n, len(match)] and take(len(match)) == match.tolist()
    for p, taken, orr in relocs:
        match, n, _ = ref.search_f_kf(oracle_mod, p, rkf, taken, orb_dist, orr)
        assert take(2) == [n, len(match)] and take(len(match)) == match.tolist()
    assert o == len(res)
