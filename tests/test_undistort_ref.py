"""CPU: cv::fisheye::undistortPoints as Frame::UndistortKeyPoints / ComputeImageBounds use it.  The restatement
(tests/undistort_ref.py) against known answers of the reference's own calibration, its planted branches, and the
library's host twin (orb_undistort_points_host, orb_image_bounds: the function the kernel compiles, with std::tan)
against the restatement, byte for byte."""
import numpy as np
import pytest

import undistort_ref as ref

f32 = np.float32


def _b(v):
    return np.asarray(v, f32).view(np.uint32)


KNOWN = [((480, 302), (480, 302)),
         ((475, 200), (474.82706, 196.47202)),
         ((100.5, 200.25), (-470.95087, 47.03491)),
         ((0, 0), (1651.294, 1038.9391)),
         ((950, 400), (-10832.09, -2056.6912))]


BIG = (1.0, 1.0, 0.0, 0.0, (0.05, 0.0, 0.0, 0.0))   # scale about 3.9 in the clip: 3e38 leaves the floats


def test_known_answers():
    for xy, want in KNOWN:
        got = ref.undistort_points(ref.YAML, [xy])[0]
        assert _b(got).tolist() == _b(want).tolist(), (xy, got.tolist(), want)


def test_known_bounds():
    got = ref.image_bounds(ref.YAML, 950, 400)
    assert _b(got).tolist() == _b([-10832.09, 5346.5034, -2056.6912, 1038.9391]).tolist(), got.tolist()


def test_clip_and_theta_past_the_pole():
    # (0, 0) of the reference's calibration: theta_d clips to pi/2 and the iteration ends beyond it, so tan is negative
    pw0, pw1, scale, iterate = ref.undistort_scale(ref.YAML, f32(0), f32(0))
    assert iterate and (pw0 * pw0 + pw1 * pw1) ** 0.5 > ref.HALF_PI and scale < 0


def test_identity_path():
    cal = (350.0, 351.0, 320.0, 240.0, (0.0, 1.0, 1.0, 1.0))
    pts = ref.seeded_points(cal, 640, 480, 64, 1)
    pts[5] = (np.nan, -np.inf)
    assert ref.undistort_points(cal, pts).tobytes() == pts.tobytes()
    assert ref.image_bounds(cal, 640, 480).tolist() == [0.0, 640.0, 0.0, 480.0]


def test_branch_at_1e_8():
    cal = ref.BRANCH
    assert ref.undistort_scale(cal, f32(3e-6), f32(0))[2:] == (1.0, False)
    assert ref.undistort_scale(cal, f32(4e-6), f32(0))[3]   # (the iteration ran, whatever its scale rounds to)
    # scale = 1: the point comes back as fx * ((x - cx) / fx) + cx rounded to float
    got = ref.undistort_points(cal, [(3e-6, 0)])[0]
    assert _b(got).tolist() == _b([f32(350.0 * (float(f32(3e-6)) / 350.0)), 0.0]).tolist()


def test_flt_min_quirk():
    # every corner lands left of x = 0 (a strongly contracting k1 around a principal point far to the left), so no
    # corner exceeds the maximum's initial value, numeric_limits<float>::min()
    cal = (5000.0, 5000.0, -5000.0, 240.0, (1.0, 0.0, 0.0, 0.0))
    corners = ref.undistort_points(cal, [(0, 0), (640, 0), (0, 480), (640, 480)])
    assert (corners[:, 0] < 0).all()
    b = ref.image_bounds(cal, 640, 480)
    assert b[1] == f32(1.17549435e-38) and b[0] == corners[:, 0].min()
    assert b[2] == corners[:, 1].min() and b[3] == corners[:, 1].max()


def test_nan_and_inf_results():
    # an infinite position makes P's third row 0 * inf: NaN, stored as 0x7FC00000 like every NaN
    un = ref.undistort_points(ref.YAML, [(np.nan, 5.0), (np.inf, 5.0), (-np.inf, 302.0)])
    assert _b(un).ravel().tolist() == [0x7FC00000] * 6
    # a result beyond the floats is an infinity with its sign
    un = ref.undistort_points(BIG, [(3e38, 0.0), (-3e38, 0.0), (0.0, -3e38)])
    assert _b(un).tolist() == _b([(np.inf, 0.0), (-np.inf, 0.0), (0.0, -np.inf)]).tolist()


def test_mild_calibration_stays_below_1_2():
    for x, y in ((0, 0), (640, 0), (0, 480), (640, 480)):
        pw0, pw1, _, _ = ref.undistort_scale(ref.MILD, f32(x), f32(y))
        assert (pw0 * pw0 + pw1 * pw1) ** 0.5 < 1.2


# ---- the library's host twin against the restatement ----

@pytest.fixture(scope="module")
def lib(orbgpu_mod):
    return orbgpu_mod


def _dist(lib, cal):
    return lib.distortion(*cal)


@pytest.mark.parametrize("name", sorted(ref.CALIBRATIONS))
def test_host_twin_equals_restatement(lib, name):
    cal = ref.CALIBRATIONS[name]
    for seed, (w, h) in enumerate(ref.IMAGE_SIZES):
        pts = ref.seeded_points(cal, w, h, 1024, 100 + seed)    # 4,096 points per calibration over the four sizes
        got = lib.undistort_points_host(_dist(lib, cal), pts)
        assert got.tobytes() == ref.undistort_points(cal, pts).tobytes(), (name, w, h)
        assert lib.image_bounds(_dist(lib, cal), w, h).tobytes() == ref.image_bounds(cal, w, h).tobytes(), (name, w, h)


def test_host_twin_known_answers_and_quirks(lib):
    d = _dist(lib, ref.YAML)
    got = lib.undistort_points_host(d, [xy for xy, _ in KNOWN])
    assert _b(got).tolist() == _b([want for _, want in KNOWN]).tolist()
    assert _b(lib.image_bounds(d, 950, 400)).tolist() == _b([-10832.09, 5346.5034, -2056.6912, 1038.9391]).tolist()
    # non-finite positions go through the arithmetic: NaN as 0x7FC00000, the infinities keep their signs
    weird = np.array([(np.nan, 5.0), (np.inf, 5.0), (-np.inf, 302.0), (5.0, np.inf)], f32)
    assert lib.undistort_points_host(d, weird).tobytes() == ref.undistort_points(ref.YAML, weird).tobytes()
    big = np.array([(3e38, 0.0), (-3e38, 0.0), (0.0, -3e38)], f32)
    assert lib.undistort_points_host(_dist(lib, BIG), big).tobytes() == ref.undistort_points(BIG, big).tobytes()
    # the identity path: bit for bit, NaN payloads included; bounds 0, w, 0, h
    ident = (350.0, 351.0, 320.0, 240.0, (0.0, 1.0, 1.0, 1.0))
    pts = ref.seeded_points(ident, 640, 480, 32, 3)
    pts.view(np.uint32)[7] = (0x7FA00001, 0xFF800000)
    assert lib.undistort_points_host(_dist(lib, ident), pts).tobytes() == pts.tobytes()
    assert lib.image_bounds(_dist(lib, ident), 640, 480).tolist() == [0.0, 640.0, 0.0, 480.0]
    # the branch and the FLT_MIN quirk
    branch = (350.0, 350.0, 0.0, 0.0, ref.YAML[4])
    pts = np.array([(3e-6, 0), (4e-6, 0), (0, -3e-6), (0, 4e-6)], f32)
    assert lib.undistort_points_host(_dist(lib, branch), pts).tobytes() == ref.undistort_points(branch, pts).tobytes()
    quirk = (5000.0, 5000.0, -5000.0, 240.0, (1.0, 0.0, 0.0, 0.0))
    b = lib.image_bounds(_dist(lib, quirk), 640, 480)
    assert b.tobytes() == ref.image_bounds(quirk, 640, 480).tobytes() and b[1] == f32(1.17549435e-38)
