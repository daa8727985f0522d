"""Pins of the projection's float forms, checked on the CPU:

* the contractions of the reference's -O3 -march=native build in Frame::isInFrustum (Frame.cc:454-456, :486) and in
  Fuse's projection (ORBmatcher.cc:859-870): tools/frustum_flags_probe.cpp, the lines written plainly and compiled with
  those flags, agrees on 10^6 random points with the explicit fmaf forms that k_project_points,
  orb_project_points_host and tests/frustum_ref.py use (tools/frustum_flags_check.cpp, built -ffp-contract=off), and
  the uncontracted forms differ, so the pin says something;
* the level thresholds of MapPoint::PredictScale: #{k : r >= T[k]} equals the direct ceilf(logf(r) / lsf) clamp for
  every float within 4,096 ulps of each threshold and for 10^6 log-uniform ratios in [2^-4, 2^8], for scale factors
  1.2f, 1.1f and 2.0f at 8 levels, with this host's libm; and the library's thresholds are those."""
import json
import os
import subprocess

import numpy as np
import pytest

import frustum_ref as ref
from test_trig_pin import TOOLS, _build, _toolchain, needs_fma


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    # -march=x86-64-v3 stands for the reference's -march=native on an AVX2+FMA host (CMakeLists.txt:10-11)
    d = str(tmp_path_factory.mktemp("frustum"))
    return _build(d, "chk", [
        ["g++", "-O3", "-march=x86-64-v3", "-std=c++11", "-c", os.path.join(TOOLS, "frustum_flags_probe.cpp"), "-o",
         "probe.o"],
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-c", os.path.join(TOOLS, "frustum_flags_check.cpp"), "-o",
         "check.o"],
        ["g++", "-o", "chk", "check.o", "probe.o", "-lm"]])


@needs_fma
def test_projection_contraction_forms(checker):
    print("pin scope:", _toolchain())
    out = json.loads(subprocess.check_output([checker, "1000000"], timeout=600))
    print(out)
    assert out["cases"] == 1_000_000 and out["kept_frame"] > 300_000 and out["kept_fuse"] > 300_000
    assert out["frame_mismatch"] == 0 and out["fuse_mismatch"] == 0 and out["kept_mismatch"] == 0
    # the contractions are real: the plain sums differ in the last bit somewhere, and the two u forms are not one
    assert out["frame_u_uncontracted_differs"] > 0 and out["fuse_u_uncontracted_differs"] > 0
    assert out["frame_ur_uncontracted_differs"] > 0 and out["fuse_ur_uncontracted_differs"] > 0
    assert out["frame_u_differs_from_fuse_u"] > 0


def test_level_thresholds_equal_the_direct_form(checker):
    print("pin scope:", _toolchain())
    out = json.loads(subprocess.check_output([checker, "levels"], timeout=600))
    print(out)
    assert out["near_cases"] == 3 * 7 * 8193 and out["uniform_cases"] == 3_000_000
    assert out["near_mismatch"] == 0 and out["uniform_mismatch"] == 0


def test_library_levels_equal_the_direct_form_around_every_threshold(orbgpu_mod):
    """The library's own thresholds (orbgpu::level_thresholds, through orb_project_points_host): a point at distance 1
    in front of the identity camera has ratio = max_dist, so its level is the library's level of that ratio; compared
    with the direct clamp (this host's logf) for every float within 4,096 ulps of each threshold."""
    import frustum_cases as fc
    for sf in (1.2, 1.1, 2.0):
        lsf = ref.logf(np.float32(sf))
        scale = np.float32(sf) ** np.arange(8, dtype=np.float32)
        cam = fc.cam_struct(orbgpu_mod, dict(fc.PLANT_CAM, scale_factors=scale, log_scale_factor=lsf))
        T = ref.level_thresholds(lsf, 8)
        bits = np.concatenate([int(np.array([t], np.float32).view(np.uint32)[0]) + np.arange(-4096, 4097) for t in T])
        ratios = bits.astype(np.uint32).view(np.float32)
        n = len(ratios)
        pos = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
        got = orbgpu_mod.project_points_host(1, cam, pos, pos, np.zeros(n, np.float32), ratios, th=1.0)
        assert (got["verdict"] == 0).all() and n == 7 * 8193
        want = np.array([ref.level_of_ratio(r, lsf, 8) for r in ratios], np.int32)
        assert np.array_equal(got["level"], want), sf
        assert set(want) == set(range(8))


def test_restatement_thresholds_and_levels_agree():
    """frustum_ref's own thresholds (ctypes logf) around each threshold: the counting rule is its direct clamp."""
    for sf in (1.2, 1.1, 2.0):
        lsf = ref.logf(np.float32(sf))
        T = ref.level_thresholds(lsf, 8)
        for k, t in enumerate(T):
            b = int(np.array([t], np.float32).view(np.uint32)[0])
            for d in (-2, -1, 0, 1, 2):
                r = np.array([b + d], np.uint32).view(np.float32)[0]
                assert sum(r >= x for x in T) == ref.level_of_ratio(r, lsf, 8), (sf, k, d)
