"""CPU: the argument checks of the undistort entry points.  Every refusal is ORB_ERR_ARG with its own message, made
before the context is touched (the context handed in is NULL: a call that got as far as the context would say "NULL
context"), and no output is written (sentinels).  n == 0 / nframes == 0 is ORB_OK without a context."""
import ctypes

import numpy as np
import pytest

import undistort_ref as ref

ERR_ARG = -1
SENT = 0x5A


@pytest.fixture(scope="module")
def L(orbgpu_mod):
    from orbgpu import _lib
    return _lib.lib()


def _dist(cal=ref.YAML, **over):
    import orbgpu
    d = orbgpu.distortion(*cal)
    for name, v in over.items():
        if name.startswith("k"):
            d.k[int(name[1])] = v
        else:
            setattr(d, name, v)
    return d


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _last(L):
    return (L.orb_last_error() or b"").decode()


BAD_DIST = [("fx", 0.0), ("fy", 0.0), ("fx", float("inf")), ("fy", float("nan")), ("cx", float("nan")),
            ("cy", float("-inf")), ("k0", float("nan")), ("k1", float("inf")), ("k2", float("nan")),
            ("k3", float("-inf"))]


class Calls:
    """One call of every entry point with valid arguments except what a test overrides; the outputs carry sentinels."""

    def __init__(self, L):
        import orbgpu
        self.L = L
        self.kps = np.zeros(4, orbgpu.KP_DTYPE)
        self.kps["x"], self.kps["y"] = [10, 20, 30, 40], [5, 6, 7, 8]
        self.xy = np.array([(10, 5), (20, 6), (30, 7), (40, 8)], np.float32)
        self.reset()

    def reset(self):
        self.xy_out = np.full((4, 2), np.float32(-77.0))
        self.kps_out = np.full(4 * 28, SENT, np.uint8)
        self.b = [ctypes.c_float(-77.0) for _ in range(4)]
        self.redone = ctypes.c_int(-77)
        self.handles = (ctypes.c_void_p * 4)(*([0x5A5A] * 4))
        self.handle = ctypes.c_void_p(0x5A5A)

    def untouched(self):
        return ((self.xy_out == np.float32(-77.0)).all() and (self.kps_out == SENT).all() and
                all(v.value == -77.0 for v in self.b) and self.redone.value == -77 and
                all(h == 0x5A5A for h in self.handles) and self.handle.value == 0x5A5A)

    def points_host(self, d, n=4, xy=True, out=True):
        return self.L.orb_undistort_points_host(d, n, _p(self.xy) if xy else None, _p(self.xy_out) if out else None)

    def bounds(self, d, w=640, h=480, null=None):
        ptrs = [None if i == null else ctypes.byref(v) for i, v in enumerate(self.b)]
        return self.L.orb_image_bounds(d, w, h, *ptrs)

    def keypoints(self, d, n=4, kps=None, out=True):
        k = self.kps if kps is None else kps
        return self.L.orb_undistort_keypoints(None, d, n, _p(k) if k is not False else None,
                                              _p(self.kps_out) if out else None, ctypes.byref(self.redone))

    def device(self, d, nframes=1, kp_cap=4, null=None):
        a = [ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)]   # never dereferenced
        if null is not None:
            a[null] = None
        return self.L.orb_undistort_keypoints_device(None, d, nframes, a[0], a[1], kp_cap, a[2],
                                                     ctypes.byref(self.redone))

    def from_extract(self, d, n=4, grid=(0.0, 0.0, 0.1, 0.1), null=None, out=True):
        a = [ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)]
        if null is not None:
            a[null] = None
        return self.L.orb_frame_create_from_extract(None, d, n, a[0], a[1], None, *grid,
                                                    ctypes.byref(self.handle) if out else None)

    def from_batch(self, d, nframes=2, kp_cap=4, grid=(0.0, 0.0, 0.1, 0.1), null=None, out=True):
        a = [ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)]
        if null is not None:
            a[null] = None
        return self.L.orb_frames_create_from_batch(None, d, nframes, a[0], a[1], a[2], kp_cap, *grid,
                                                   self.handles if out else None)

    def all(self):
        return [self.points_host, self.bounds, self.keypoints, self.device, self.from_extract, self.from_batch]


@pytest.fixture()
def C(L):
    return Calls(L)


def _refused(C, status, needle):
    assert status == ERR_ARG, status
    msg = _last(C.L)
    assert needle in msg and "NULL context" not in msg, msg
    assert C.untouched(), msg
    C.reset()


def test_null_dist(C):
    for call in C.all():
        _refused(C, call(None), "dist NULL")


@pytest.mark.parametrize("field,value", BAD_DIST)
def test_bad_calibration(C, field, value):
    d = _dist(**{field: value})
    needle = {"f": "fx or fy", "c": "cx or cy", "k": "coefficient"}[field[0]]
    for call in C.all():
        _refused(C, call(ctypes.byref(d)), needle)


def test_negative_counts(C):
    d = ctypes.byref(_dist())
    _refused(C, C.points_host(d, n=-1), "n < 0")
    _refused(C, C.keypoints(d, n=-1), "n < 0")
    _refused(C, C.from_extract(d, n=-1), "n < 0")
    _refused(C, C.device(d, nframes=-1), "nframes < 0")
    _refused(C, C.from_batch(d, nframes=-1), "nframes < 0")
    _refused(C, C.bounds(d, w=-1), "negative image size")
    _refused(C, C.bounds(d, h=-1), "negative image size")


def test_null_arrays(C):
    d = ctypes.byref(_dist())
    _refused(C, C.points_host(d, xy=False), "NULL arrays")
    _refused(C, C.points_host(d, out=False), "NULL arrays")
    _refused(C, C.keypoints(d, kps=False), "NULL arrays")
    _refused(C, C.keypoints(d, out=False), "NULL arrays")
    for i in range(3):
        _refused(C, C.device(d, null=i), "NULL arrays")
        _refused(C, C.from_batch(d, null=i), "NULL arrays")
    _refused(C, C.from_batch(d, out=False), "NULL arrays")
    for i in range(2):
        _refused(C, C.from_extract(d, null=i), "NULL arrays")
    _refused(C, C.from_extract(d, out=False), "out NULL")
    for i in range(4):
        _refused(C, C.bounds(d, null=i), "NULL output")


def test_kp_cap_below_one(C):
    d = ctypes.byref(_dist())
    for cap in (0, -3):
        _refused(C, C.device(d, kp_cap=cap), "kp_cap < 1")
        _refused(C, C.from_batch(d, kp_cap=cap), "kp_cap < 1")


@pytest.mark.parametrize("grid,needle", [((0.0, 0.0, 0.0, 0.1), "inverse cell size"),
                                         ((0.0, 0.0, 0.1, -1.0), "inverse cell size"),
                                         ((0.0, 0.0, float("nan"), 0.1), "inverse cell size"),
                                         ((0.0, 0.0, 0.1, float("inf")), "inverse cell size"),
                                         ((float("nan"), 0.0, 0.1, 0.1), "grid origin"),
                                         ((0.0, float("inf"), 0.1, 0.1), "grid origin")])
def test_grid_checks(C, grid, needle):
    d = ctypes.byref(_dist())
    _refused(C, C.from_extract(d, grid=grid), needle)
    _refused(C, C.from_batch(d, grid=grid), needle)


@pytest.mark.parametrize("field,value", [("x", float("nan")), ("y", float("inf")), ("x", float("-inf"))])
def test_host_keypoint_not_finite(C, field, value):
    k = C.kps.copy()
    k[field][2] = value
    _refused(C, C.keypoints(ctypes.byref(_dist()), kps=k), "keypoint position not finite")


def test_zero_is_ok_without_a_context(C):
    d = ctypes.byref(_dist())
    assert C.points_host(d, n=0, xy=False, out=False) == 0
    assert C.keypoints(d, n=0, kps=False, out=False) == 0 and C.redone.value == 0
    C.reset()
    assert C.device(d, nframes=0, kp_cap=0) == 0 and C.redone.value == 0
    C.reset()
    assert C.from_batch(d, nframes=0, kp_cap=0, out=False) == 0
    assert C.untouched()
    assert C.bounds(d, w=0, h=0) == 0


def test_valid_arguments_reach_the_context(C):
    # the same calls with nothing wrong are refused only for their NULL context: the checks above are not vacuous
    d = ctypes.byref(_dist())
    for call in (C.keypoints, C.device, C.from_extract, C.from_batch):
        assert call(d) == ERR_ARG and "NULL context" in _last(C.L)
        assert C.untouched()
    assert C.L.orb_debug_undistort_guard(None, 0.0) == ERR_ARG
