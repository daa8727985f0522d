"""CPU: what orb_search_by_match_bird and orb_search_by_match_bird_frame refuse.  The arguments are checked before
the context is touched, so a NULL context (no GPU here) shows it: every malformed call is ORB_ERR_ARG with its own
message and the outputs untouched, and a well-formed one gets as far as the NULL-context error."""
import ctypes

import numpy as np
import pytest

N = 10
SENTINEL = 77


@pytest.fixture()
def env(orbgpu_mod):
    from orbgpu import _lib
    e = dict(L=_lib.lib(), lib=_lib)
    e["desc"] = np.zeros((N, 32), np.uint8)
    e["kps"] = np.zeros(N, orbgpu_mod.KP_DTYPE)
    e["xy"] = np.full((N, 2), 50.0, np.float32)
    e["ang"] = np.zeros(N, np.float32)
    e["ids"] = np.arange(N, dtype=np.int32)
    e["off"] = np.zeros(64 * 48 + 1, np.int32)
    e["off"][5:] = N   # cell 4 holds all ten keypoints
    e["idx"] = np.arange(N, dtype=np.int32)
    e["mp"] = np.ones(N, np.uint8)
    return e


def _kf(e, **kw):
    a = dict(ctx=None, nnratio=0.8, check_ori=1, max_dist=100, r=10.0, nq=N, ids=e["ids"], xy=e["xy"], ang=e["ang"],
             qdesc=e["desc"], nt=N, tdesc=e["desc"], kps=e["kps"], off=e["off"], idx=e["idx"], out=True)
    a.update(kw)
    p = lambda v: None if v is None else v.ctypes.data   # noqa: E731
    match = np.full(N, SENTINEL, np.int32)
    nm = ctypes.c_int(SENTINEL)
    g = e["lib"].OrbFrameGrid(0.0, 0.0, 0.1, 0.1, p(a["off"]), p(a["idx"]))
    st = e["L"].orb_search_by_match_bird(a["ctx"], a["nnratio"], a["check_ori"], a["max_dist"], a["r"], a["nq"],
                                         p(a["ids"]), p(a["xy"]), p(a["ang"]), p(a["qdesc"]), a["nt"], p(a["tdesc"]),
                                         p(a["kps"]), g, match.ctypes.data if a["out"] else None, ctypes.byref(nm))
    assert (match == SENTINEL).all() and nm.value == SENTINEL, "an output was written"
    return st, e["L"].orb_last_error().decode()


def _frame(e, **kw):
    a = dict(n_last=N, dl=e["desc"], kl=e["kps"], mp=e["mp"], n_cur=N, dc=e["desc"], kc=e["kps"], off=e["off"],
             idx=e["idx"], out=True)
    a.update(kw)
    p = lambda v: None if v is None else v.ctypes.data   # noqa: E731
    match = np.full(N, SENTINEL, np.int32)
    nm = ctypes.c_int(SENTINEL)
    g = e["lib"].OrbFrameGrid(0.0, 0.0, 0.1, 0.1, p(a["off"]), p(a["idx"]))
    st = e["L"].orb_search_by_match_bird_frame(None, 0.9, 1, 15.0, a["n_last"], p(a["dl"]), p(a["kl"]), p(a["mp"]),
                                               a["n_cur"], p(a["dc"]), p(a["kc"]), g,
                                               match.ctypes.data if a["out"] else None, ctypes.byref(nm))
    assert (match == SENTINEL).all() and nm.value == SENTINEL, "an output was written"
    return st, e["L"].orb_last_error().decode()


def _with(a, i, v):
    b = a.copy()
    b.flat[i] = v
    return b


def test_keyframe_form_refusals(env):
    e = env
    assert _kf(e) == (-1, "NULL context")
    assert _kf(e, nq=0) == (-1, "NULL context")   # (nothing is written either)
    assert _kf(e, nt=0, off=np.zeros(64 * 48 + 1, np.int32)) == (-1, "NULL context")
    assert _kf(e, nt=0) == (-1, "orb_search_by_match_bird: grid index out of range")   # a grid of ten, no trains
    name = "orb_search_by_match_bird: "
    for bad in (np.nan, np.inf, -np.inf):
        assert _kf(e, xy=_with(e["xy"], 7, bad)) == (-1, name + "query centre not finite")
        assert _kf(e, r=float(bad)) == (-1, name + "radius not finite or negative")
    assert _kf(e, r=-0.5) == (-1, name + "radius not finite or negative")
    for md in (-1, 257):
        assert _kf(e, max_dist=md) == (-1, name + "max_dist outside [0, 256]")
    for kw in (dict(xy=None), dict(qdesc=None), dict(ang=None), dict(tdesc=None), dict(kps=None), dict(out=False),
               dict(off=None), dict(idx=None), dict(nq=-1), dict(nt=-1)):
        assert _kf(e, **kw) == (-1, name + "bad arguments"), kw
    assert _kf(e, ang=None, check_ori=0) == (-1, "NULL context")   # the angles are read with check_ori only
    assert _kf(e, ids=None) == (-1, "NULL context")                # NULL ids: the query's position is its id
    assert _kf(e, ids=_with(e["ids"], 3, -1)) == (-1, name + "negative query id")
    assert _kf(e, off=_with(e["off"], 0, 1)) == (-1, name + "grid cell_off[0] != 0")
    assert _kf(e, off=_with(e["off"], 100, 3)) == (-1, name + "grid cell_off decreases")
    assert _kf(e, idx=_with(e["idx"], 7, N)) == (-1, name + "grid index out of range")
    assert _kf(e, idx=_with(e["idx"], 2, -1)) == (-1, name + "grid index out of range")
    assert _kf(e, max_dist=0) == (-1, "NULL context") and _kf(e, max_dist=256, r=0.0) == (-1, "NULL context")


def test_grid_is_checked_before_the_query_values(env):
    """The Frame grid is checked with the other pointers, ahead of the per-query values: a call with two faults
    reports the grid's (a NULL one as "bad arguments")."""
    e, name = env, "orb_search_by_match_bird: "
    nan_xy, neg_id = _with(e["xy"], 7, np.nan), _with(e["ids"], 3, -1)
    assert _kf(e, xy=nan_xy, off=_with(e["off"], 100, 3)) == (-1, name + "grid cell_off decreases")
    assert _kf(e, ids=neg_id, idx=_with(e["idx"], 7, N)) == (-1, name + "grid index out of range")
    assert _kf(e, xy=nan_xy, off=None) == (-1, name + "bad arguments")
    assert _kf(e, r=np.nan, off=_with(e["off"], 0, 1)) == (-1, name + "radius not finite or negative")   # (a scalar)


def test_frame_form_refusals(env):
    e = env
    assert _frame(e) == (-1, "NULL context")
    assert _frame(e, mp=None) == (-1, "NULL context")
    name = "orb_search_by_match_bird_frame: "
    for kw in (dict(dl=None), dict(kl=None), dict(dc=None), dict(kc=None), dict(out=False), dict(off=None),
               dict(idx=None), dict(n_last=-1), dict(n_cur=-1)):
        assert _frame(e, **kw) == (-1, name + "bad arguments"), kw
    assert _frame(e, off=_with(e["off"], 0, 1)) == (-1, name + "grid cell_off[0] != 0")
    assert _frame(e, off=_with(e["off"], 100, 3)) == (-1, name + "grid cell_off decreases")
    assert _frame(e, idx=_with(e["idx"], 7, N)) == (-1, name + "grid index out of range")
