"""GPU parity of Frame::ComputeStereoMatches (k_stereo_bucket / k_stereo / k_stereo_cut, csrc/stereo.hip) against
tests/stereo_ref.py on the planted cases of tests/stereo_cases.py: mvuRight / mvDepth byte for byte and the match
count, reading the right image in place and from the staging copy (ORBGPU_STEREO_STAGE=1).  tests/test_stereo_cases.py
checks on the CPU that the cases realise every decision they are named for and keep every window read inside its
level image."""
import ctypes

import numpy as np
import pytest

import stereo_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["in_place", "staged"])
def staging(request, monkeypatch):
    if request.param == "staged":
        monkeypatch.setenv("ORBGPU_STEREO_STAGE", "1")
    else:
        monkeypatch.delenv("ORBGPU_STEREO_STAGE", raising=False)
    return request.param


def _extractors(orbgpu_mod, c):
    p = c.params
    return [orbgpu_mod.ORBextractor(p["nfeatures"], p["scaleFactor"], p["nlevels"], p["iniThFAST"], p["minThFAST"])
            for _ in range(2)]


def _run(orbgpu_mod, oracle_mod, gl, gr, name, check_levels=False):
    c = sc.case(name)
    want_u, want_d, want_n, _, ll, lr, _ = sc.expected(oracle_mod, name)
    gl(c.left)       # the case's own arrays: their row stride goes down as it is
    gr(c.right)
    if check_levels:
        for l in (0, c.params["nlevels"] - 1):
            assert np.array_equal(gl.debug_level_image(l), ll[l]) and np.array_equal(gr.debug_level_image(l), lr[l]), l
    u, d, n = orbgpu_mod.compute_stereo_matches(gl, gr, c.kl, c.dl, c.kr, c.dr, c.mb, c.mbf)
    bad = np.flatnonzero(u.view(np.uint32) != want_u.view(np.uint32))[:8]
    assert bad.size == 0, (name, bad.tolist(), u[bad].tolist(), want_u[bad].tolist())
    assert d.tobytes() == want_d.tobytes(), name
    assert n == want_n, (name, n, want_n)


@pytest.mark.parametrize("name", sc.CASES)
def test_planted_cases_match_reference(orbgpu_mod, oracle_mod, staging, name):
    gl, gr = _extractors(orbgpu_mod, sc.case(name))
    _run(orbgpu_mod, oracle_mod, gl, gr, name, check_levels=True)


def test_back_to_back_on_one_context_pair(orbgpu_mod, oracle_mod, staging):
    """A larger call, then smaller ones, on the same two contexts: the staging arena is reused and must not show
    the earlier call's keypoints, window distances or row buckets."""
    gl, gr = _extractors(orbgpu_mod, sc.case("many"))
    for name in ("big_nr", "many", "median_zero", "nl_one", "nr_zero", "search"):
        _run(orbgpu_mod, oracle_mod, gl, gr, name)


def test_too_many_right_keypoints_is_an_argument_error(orbgpu_mod, oracle_mod):
    """nR above 2^24 - 1 is refused before anything is read or launched.  The arrays here hold one keypoint, so if
    the check were lost the host copy of nR keypoints would read far past them and the process would die, not fail
    an assertion: an allocation of 2^24 keypoints and descriptors (1 GB) is the price of a clean failure."""
    c = sc.case("nl_one")
    gl, gr = _extractors(orbgpu_mod, c)
    gl(c.left)
    gr(c.right)
    L = orbgpu_mod._lib.lib()
    kl, dl, kr, dr = (np.ascontiguousarray(a) for a in (c.kl, c.dl, c.kr, c.dr))
    u, d = np.full(1, 7, np.float32), np.full(1, 7, np.float32)
    n = ctypes.c_int(-5)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    for nr, status in ((1 << 24, -1), ((1 << 31) - 1, -1)):
        st = L.orb_compute_stereo_matches(gl.h, gr.h, 1, p(kl), p(dl), nr, p(kr), p(dr), c.mb, c.mbf, p(u), p(d),
                                          ctypes.byref(n))
        assert st == status and u[0] == 7 and d[0] == 7 and n.value == -5, (nr, st)
    _run(orbgpu_mod, oracle_mod, gl, gr, "nl_one")      # the contexts still work after the refusal
