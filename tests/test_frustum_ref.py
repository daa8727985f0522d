"""CPU: the planted decisions of Frame::isInFrustum, Fuse's projection and PredictScale on the restatement
(tests/frustum_ref.py), one hand-built point per branch and per side of each comparison (tests/frustum_cases.py), and
the library's host form of the projection (orb_project_points_host: the function the kernel compiles) against the
restatement, byte for byte, on the planted points and on a random shell."""
import numpy as np
import pytest

import frustum_cases as fc
import frustum_ref as ref

f32 = np.float32


def _run(mode, p, th=1.0):
    name, pos, normal, lo, hi = p[:5]
    if mode == 0:
        return ref.is_in_frustum(fc.PLANT_CAM, pos, normal, lo, hi, 0.5, th)
    return ref.fuse_projection(fc.PLANT_CAM, pos, normal, lo, hi, th)


def test_planted_points_are_what_they_claim():
    P = {p[0]: p for p in fc.planted()}
    T = fc.thresholds()
    assert len(T) == fc.NLEVELS - 1 and all(np.isfinite(t) for t in T) and list(T) == sorted(T)
    assert T[0] == fc.up(1.0)                                      # ceil(logf(r) / lsf) > 0 from the float after 1
    assert f32(f32(0.8) * P["dist_at_min"][3]) == f32(4.0) < f32(f32(0.8) * P["dist_below_min"][3])
    assert f32(f32(1.2) * P["dist_at_max"][4]) == f32(6.0) > f32(f32(1.2) * P["dist_above_max"][4])
    assert float(P["cos_above_0998"][2][2]) > 0.998 > float(P["cos_below_0998"][2][2])
    assert f32(512.0) * f32(0.625) + f32(320.0) == f32(640.0)


@pytest.mark.parametrize("mode", [0, 1], ids=["frame", "fuse"])
def test_planted_verdicts(mode):
    seen = set()
    for p in fc.planted():
        rec = _run(mode, p)
        assert rec["verdict"] == p[5 + mode], (p[0], rec)
        seen.add(rec["verdict"])
        if rec["verdict"] not in (ref.VISIBLE, ref.NOT_FINITE):   # (verdict 5 comes after everything was computed)
            assert rec["level"] == -1 and rec["r"] == 0, p[0]
    assert seen >= {ref.VISIBLE, ref.DEPTH, ref.BOUNDS, ref.DISTANCE, ref.ANGLE}
    if mode == 0:
        assert ref.NOT_FINITE in seen


def test_planted_bounds_values():
    P = {p[0]: p for p in fc.planted()}
    for mode in (0, 1):
        assert _run(mode, P["u_max"])["u"] == f32(640.0) and _run(mode, P["u_min"])["u"] == f32(0.0)
        assert _run(mode, P["v_max"])["v"] == f32(480.0) and _run(mode, P["v_min"])["v"] == f32(0.0)
        assert _run(mode, P["u_above_max"])["u"] > f32(640.0) and _run(mode, P["u_below_min"])["u"] < f32(0.0)
        assert _run(mode, P["dist_at_min"])["dist"] == f32(4.0) and _run(mode, P["dist_at_max"])["dist"] == f32(6.0)
    assert _run(0, P["cos_at_limit"])["view_cos"] == f32(0.5) > _run(0, P["cos_below_limit"])["view_cos"]
    nan = _run(0, P["z_0_x_0"])
    assert np.isnan(nan["u"]) and np.isinf(nan["invz"]) and nan["dist"] == 0 and nan["level"] == 0


@pytest.mark.parametrize("th", [1.0, 3.0])
def test_planted_levels_and_radii(th):
    for p in fc.planted():
        name, level, r0 = p[0], p[7], p[8]
        a, b = _run(0, p, th), _run(1, p, th)
        if level is not None:
            assert a["level"] == level and b["level"] == level, name
            assert b["r"] == f32(f32(th) * fc.SCALE[level]), name
        if r0 is not None:
            want = f32(r0) if th == 1.0 else f32(f32(r0) * f32(th))   # `if(th!=1.0) r*=th`
            assert a["r"] == f32(want * fc.SCALE[a["level"]]), name
            assert a["ur"] == f32(a["u"] - f32(40.0) * a["invz"]), name   # invz = 1: the product is exact


def test_negative_zero_depth_passes_the_depth_test():
    """PcZ == -0.0 is not < 0.0f: invz = -inf, u is NaN; FRAME ends in verdict 5, Fuse's IsInImage rejects."""
    cam = dict(fc.PLANT_CAM, tcw=np.array([-0.0, -0.0, -0.0], f32))
    pos, z = np.array([-0.0, -0.0, -0.0], f32), np.array([0, 0, 1], f32)
    a = ref.is_in_frustum(cam, pos, z, 0.0, 1.0, 0.5, 1.0)
    assert np.signbit(a["invz"]) and np.isinf(a["invz"]) and a["verdict"] == ref.NOT_FINITE
    assert ref.fuse_projection(cam, pos, z, 0.0, 1.0, 3.0)["verdict"] == ref.BOUNDS


def test_level_rule_outside_the_finite_ratios():
    for ratio in (np.inf, -np.inf, np.nan, -1.0, 0.0):
        assert ref.level_of_ratio(f32(ratio), fc.LSF, 8) == 0
    assert ref.level_of_ratio(f32(3.0e38), fc.LSF, 8) == 7 and ref.level_of_ratio(f32(1e-40), fc.LSF, 8) == 0


def _host(orbgpu_mod, mode, cam, arrays, th, limit=0.5):
    return orbgpu_mod.project_points_host(mode, fc.cam_struct(orbgpu_mod, cam), *arrays, view_cos_limit=limit, th=th)


@pytest.mark.parametrize("mode", [0, 1], ids=["frame", "fuse"])
@pytest.mark.parametrize("th", [1.0, 3.0])
def test_host_projection_equals_the_restatement_on_the_planted_points(orbgpu_mod, mode, th):
    arrays = fc.arrays(fc.planted())
    want = ref.as_array(ref.project(mode, fc.PLANT_CAM, *arrays, view_cos_limit=0.5, th=th), orbgpu_mod.POINT_PROJ_DTYPE)
    got = _host(orbgpu_mod, mode, fc.PLANT_CAM, arrays, th)
    for k in ref.FIELDS:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


@pytest.mark.parametrize("mode", [0, 1], ids=["frame", "fuse"])
def test_host_projection_equals_the_restatement_on_a_random_shell(orbgpu_mod, mode):
    cam = fc.make_camera(3)
    arrays = fc.random_points(17, 600, cam)
    want = ref.as_array(ref.project(mode, cam, *arrays, view_cos_limit=0.5, th=3.0), orbgpu_mod.POINT_PROJ_DTYPE)
    counts = np.bincount(want["verdict"], minlength=6)
    assert (counts[:5] >= 0.05 * len(want)).all(), counts
    assert len(set(want["level"][want["verdict"] == 0])) == fc.NLEVELS
    got = _host(orbgpu_mod, mode, cam, arrays, 3.0)
    assert got.tobytes() == want.tobytes()
