"""CPU: what the grid searches refuse, and in which order, for both forms of the train side: host arrays with a Frame
grid (orb_search_by_projection, orb_window_match_grid) and a resident frame (orb_search_by_projection_frame,
orb_window_match_frame, orb_search_by_match_bird_resident; the match-bird host forms are in
test_match_bird_args_cpu.py).  The arguments are checked before the context is touched, so a NULL context (no GPU
here) shows it.  Every row is one malformed call: ORB_ERR_ARG, its exact orb_last_error() text, the outputs untouched,
and then the well-formed call, which gets as far as "NULL context".  The resident forms are given a NULL frame (a
handle needs a device), so "NULL frame" is as far as their well-formed call gets, and a row with a second fault shows
which of the two is reported."""
import ctypes

import numpy as np
import pytest

NQ, NT = 4, 10
SENTINEL = 77
ORB_ERR_ARG = -1
CELLS = 64 * 48


@pytest.fixture()
def env(orbgpu_mod):
    from orbgpu import _lib
    e = dict(L=_lib.lib(), lib=_lib)
    q = np.zeros(NQ, orbgpu_mod.PROJ_QUERY_DTYPE)
    q["u"], q["v"], q["r"], q["min_level"], q["max_level"] = 50.0, 50.0, 5.0, -1, -1
    e["q"] = q
    e["qdesc"] = np.zeros((NQ, 32), np.uint8)
    e["kq"] = np.zeros(NQ, orbgpu_mod.KP_DTYPE)
    e["cen"] = np.full((NQ, 2), 50.0, np.float32)
    e["xy"] = np.full((NQ, 2), 50.0, np.float32)
    e["ang"] = np.zeros(NQ, np.float32)
    e["ids"] = np.arange(NQ, dtype=np.int32)
    e["tdesc"] = np.zeros((NT, 32), np.uint8)
    e["kt"] = np.zeros(NT, orbgpu_mod.KP_DTYPE)
    e["ur"] = np.full(NT, -1.0, np.float32)
    e["taken"] = np.zeros(NT, np.uint8)
    e["off"] = np.zeros(CELLS + 1, np.int32)
    e["off"][5:] = NT   # cell 4 holds all ten trains
    e["idx"] = np.arange(NT, dtype=np.int32)
    return e


def _p(v):
    return None if v is None else v.ctypes.data


def _call(e, fn, args_of, kw):
    """One call of fn with the defaults of args_of() overridden by kw -> (status, message); no output may change."""
    match = np.full(NT, SENTINEL, np.int32)
    nm = ctypes.c_int(SENTINEL)
    st = getattr(e["L"], fn)(*args_of(e, match, nm, kw))
    assert (match == SENTINEL).all() and nm.value == SENTINEL, "an output was written"
    return st, e["L"].orb_last_error().decode()


def _grid(e, a):
    return e["lib"].OrbFrameGrid(0.0, 0.0, 0.1, 0.1, _p(a["off"]), _p(a["idx"]))


def _proj_args(e, match, nm, kw):
    a = dict(mode=0, max_dist=100, nq=NQ, q=e["q"], qdesc=e["qdesc"], nt=NT, tdesc=e["tdesc"], kps=e["kt"], ur=e["ur"],
             taken=e["taken"], off=e["off"], idx=e["idx"], out=True)
    a.update(kw)
    return (None, a["mode"], 0.8, 1, a["max_dist"], a["nq"], _p(a["q"]), _p(a["qdesc"]), a["nt"], _p(a["tdesc"]),
            _p(a["kps"]), _p(a["ur"]), _p(a["taken"]), _grid(e, a), match.ctypes.data if a["out"] else None,
            ctypes.byref(nm))


def _window_args(e, match, nm, kw):
    a = dict(n1=NQ, desc1=e["qdesc"], kps1=e["kq"], cen=e["cen"], window=10.0, n2=NT, desc2=e["tdesc"], kps2=e["kt"],
             off=e["off"], idx=e["idx"], out=True)
    a.update(kw)
    return (None, 0.9, 1, 0, a["n1"], _p(a["desc1"]), _p(a["kps1"]), _p(a["cen"]), a["window"], a["n2"],
            _p(a["desc2"]), _p(a["kps2"]), _grid(e, a), match.ctypes.data if a["out"] else None, ctypes.byref(nm))


def _proj_frame_args(e, match, nm, kw):
    a = dict(mode=0, max_dist=100, nq=NQ, q=e["q"], qdesc=e["qdesc"], taken=e["taken"], use_ur=0, out=True)
    a.update(kw)
    return (None, a["mode"], 0.8, 1, a["max_dist"], a["nq"], _p(a["q"]), _p(a["qdesc"]), None, _p(a["taken"]),
            a["use_ur"], match.ctypes.data if a["out"] else None, ctypes.byref(nm))


def _window_frame_args(e, match, nm, kw):
    a = dict(n1=NQ, desc1=e["qdesc"], kps1=e["kq"], cen=e["cen"], window=10.0, out=True)
    a.update(kw)
    return (None, 0.9, 1, 0, a["n1"], _p(a["desc1"]), _p(a["kps1"]), _p(a["cen"]), a["window"], None,
            match.ctypes.data if a["out"] else None, ctypes.byref(nm))


def _bird_resident_args(e, match, nm, kw):
    a = dict(check_ori=1, max_dist=100, r=10.0, nq=NQ, ids=e["ids"], xy=e["xy"], ang=e["ang"], qdesc=e["qdesc"],
             out=True)
    a.update(kw)
    return (None, 0.8, a["check_ori"], a["max_dist"], a["r"], a["nq"], _p(a["ids"]), _p(a["xy"]), _p(a["ang"]),
            _p(a["qdesc"]), None, match.ctypes.data if a["out"] else None, ctypes.byref(nm))


# entry point -> (its arguments, how far its well-formed call gets without a device)
FORMS = {
    "orb_search_by_projection": (_proj_args, "NULL context"),
    "orb_window_match_grid": (_window_args, "NULL context"),
    "orb_search_by_projection_frame": (_proj_frame_args, "orb_search_by_projection_frame: NULL frame"),
    "orb_window_match_frame": (_window_frame_args, "orb_window_match_frame: NULL frame"),
    "orb_search_by_match_bird_resident": (_bird_resident_args, "orb_search_by_match_bird_resident: NULL frame"),
}


def _set(key, i, v):
    """The env array `key` with element i (a flat index, or (field, index) of a record array) set to v."""
    def make(e):
        b = e[key].copy()
        if isinstance(i, tuple):
            b[i[0]][i[1]] = v
        else:
            b.flat[i] = v
        return b
    return make


NAN, INF = float("nan"), float("inf")
BAD = "bad arguments"
MODE, MAXD = "unknown mode", "max_dist outside [0, 256]"
WIN = "query window not finite or radius negative"
RADIUS = "radius not finite or negative"
OFF0, DECR, RANGE = "grid cell_off[0] != 0", "grid cell_off decreases", "grid index out of range"
NOFRAME = "NULL frame"
G_OFF0, G_DECR = dict(off=_set("off", 0, 1)), dict(off=_set("off", 100, 3))
G_HIGH, G_LOW = dict(idx=_set("idx", 7, NT)), dict(idx=_set("idx", 2, -1))
Q_NAN = dict(q=_set("q", ("u", 2), NAN))

# (entry point, overrides of the well-formed call (a callable is given the env), the fault reported)
ROWS = [
    # --- orb_search_by_projection: one fault
    ("orb_search_by_projection", dict(mode=2), MODE),
    ("orb_search_by_projection", dict(mode=-1), MODE),
    ("orb_search_by_projection", dict(max_dist=-1), MAXD),
    ("orb_search_by_projection", dict(max_dist=257), MAXD),
    ("orb_search_by_projection", dict(nq=-1), BAD),
    ("orb_search_by_projection", dict(nt=-1), BAD),
    ("orb_search_by_projection", dict(out=False), BAD),
    ("orb_search_by_projection", dict(q=None), BAD),
    ("orb_search_by_projection", dict(qdesc=None), BAD),
    ("orb_search_by_projection", dict(tdesc=None), BAD),
    ("orb_search_by_projection", dict(kps=None), BAD),
    ("orb_search_by_projection", dict(off=None), BAD),
    ("orb_search_by_projection", dict(idx=None), BAD),
    ("orb_search_by_projection", G_OFF0, OFF0),
    ("orb_search_by_projection", G_DECR, DECR),
    ("orb_search_by_projection", G_HIGH, RANGE),
    ("orb_search_by_projection", G_LOW, RANGE),
    ("orb_search_by_projection", dict(nt=0), RANGE),   # a grid of ten, no trains
    ("orb_search_by_projection", Q_NAN, WIN),
    ("orb_search_by_projection", dict(q=_set("q", ("v", 0), INF)), WIN),
    ("orb_search_by_projection", dict(q=_set("q", ("v", 3), -INF)), WIN),
    ("orb_search_by_projection", dict(q=_set("q", ("r", 1), NAN)), WIN),
    ("orb_search_by_projection", dict(q=_set("q", ("r", 1), INF)), WIN),
    ("orb_search_by_projection", dict(q=_set("q", ("r", 3), -0.5)), WIN),
    # --- two faults: the scalars, then the pointers and counts, then the grid, then the queries
    ("orb_search_by_projection", dict(mode=2, max_dist=257), MODE),
    ("orb_search_by_projection", dict(mode=2, q=None), MODE),
    ("orb_search_by_projection", dict(max_dist=-1, nt=-1), MAXD),
    ("orb_search_by_projection", dict(max_dist=257, **G_DECR), MAXD),
    ("orb_search_by_projection", dict(tdesc=None, **G_OFF0), BAD),
    ("orb_search_by_projection", dict(G_DECR, **Q_NAN), DECR),
    ("orb_search_by_projection", dict(G_HIGH, q=_set("q", ("r", 0), -1.0)), RANGE),
    ("orb_search_by_projection", dict(Q_NAN, off=None), BAD),
    ("orb_search_by_projection", dict(Q_NAN, mode=3), MODE),
    # --- orb_window_match_grid: one fault
    ("orb_window_match_grid", dict(n1=-1), BAD),
    ("orb_window_match_grid", dict(n2=-1), BAD),
    ("orb_window_match_grid", dict(out=False), BAD),
    ("orb_window_match_grid", dict(desc1=None), BAD),
    ("orb_window_match_grid", dict(kps1=None), BAD),
    ("orb_window_match_grid", dict(desc2=None), BAD),
    ("orb_window_match_grid", dict(kps2=None), BAD),
    ("orb_window_match_grid", dict(off=None), BAD),
    ("orb_window_match_grid", dict(idx=None), BAD),
    ("orb_window_match_grid", G_OFF0, OFF0),
    ("orb_window_match_grid", G_DECR, DECR),
    ("orb_window_match_grid", G_HIGH, RANGE),
    ("orb_window_match_grid", G_LOW, RANGE),
    ("orb_window_match_grid", dict(n2=0), RANGE),
    # --- two faults (the centres and the window are not checked: the kernel clamps the rectangle)
    ("orb_window_match_grid", dict(desc2=None, **G_DECR), BAD),
    ("orb_window_match_grid", dict(G_OFF0, cen=_set("cen", 3, NAN)), OFF0),
    ("orb_window_match_grid", dict(G_HIGH, window=NAN), RANGE),
    # --- orb_search_by_projection_frame: mode, max_dist, then the frame, ahead of everything read through it
    ("orb_search_by_projection_frame", dict(mode=2), MODE),
    ("orb_search_by_projection_frame", dict(max_dist=-1), MAXD),
    ("orb_search_by_projection_frame", dict(max_dist=257), MAXD),
    ("orb_search_by_projection_frame", dict(mode=2, max_dist=257), MODE),
    ("orb_search_by_projection_frame", dict(nq=-1), NOFRAME),
    ("orb_search_by_projection_frame", dict(q=None), NOFRAME),
    ("orb_search_by_projection_frame", dict(qdesc=None), NOFRAME),
    ("orb_search_by_projection_frame", dict(out=False), NOFRAME),
    ("orb_search_by_projection_frame", dict(use_ur=1), NOFRAME),
    ("orb_search_by_projection_frame", Q_NAN, NOFRAME),
    ("orb_search_by_projection_frame", dict(q=_set("q", ("r", 1), -0.5)), NOFRAME),
    ("orb_search_by_projection_frame", dict(Q_NAN, mode=2), MODE),
    ("orb_search_by_projection_frame", dict(Q_NAN, max_dist=300), MAXD),
    # --- orb_window_match_frame: the frame first
    ("orb_window_match_frame", dict(n1=-1), NOFRAME),
    ("orb_window_match_frame", dict(out=False), NOFRAME),
    ("orb_window_match_frame", dict(desc1=None), NOFRAME),
    ("orb_window_match_frame", dict(kps1=None), NOFRAME),
    ("orb_window_match_frame", dict(cen=_set("cen", 0, INF), window=-1.0), NOFRAME),
    # --- orb_search_by_match_bird_resident: max_dist, the radius, then the frame
    ("orb_search_by_match_bird_resident", dict(max_dist=-1), MAXD),
    ("orb_search_by_match_bird_resident", dict(max_dist=257), MAXD),
    ("orb_search_by_match_bird_resident", dict(r=NAN), RADIUS),
    ("orb_search_by_match_bird_resident", dict(r=INF), RADIUS),
    ("orb_search_by_match_bird_resident", dict(r=-0.5), RADIUS),
    ("orb_search_by_match_bird_resident", dict(max_dist=257, r=NAN), MAXD),
    ("orb_search_by_match_bird_resident", dict(nq=-1), NOFRAME),
    ("orb_search_by_match_bird_resident", dict(xy=None), NOFRAME),
    ("orb_search_by_match_bird_resident", dict(qdesc=None), NOFRAME),
    ("orb_search_by_match_bird_resident", dict(ang=None), NOFRAME),
    ("orb_search_by_match_bird_resident", dict(out=False), NOFRAME),
    ("orb_search_by_match_bird_resident", dict(xy=_set("xy", 5, NAN)), NOFRAME),
    ("orb_search_by_match_bird_resident", dict(ids=_set("ids", 3, -1)), NOFRAME),
    ("orb_search_by_match_bird_resident", dict(xy=_set("xy", 5, INF), max_dist=-1), MAXD),
    ("orb_search_by_match_bird_resident", dict(ids=_set("ids", 3, -1), r=-1.0), RADIUS),
]


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_refusal(env, row):
    fn, kw, why = ROWS[row]
    args_of, reached = FORMS[fn]
    kw = {k: v(env) if callable(v) else v for k, v in kw.items()}
    assert _call(env, fn, args_of, kw) == (ORB_ERR_ARG, fn + ": " + why), (fn, sorted(kw))
    assert _call(env, fn, args_of, {}) == (ORB_ERR_ARG, reached), fn


@pytest.mark.parametrize("fn", ["orb_search_by_projection", "orb_window_match_grid"])
def test_well_formed_variants_reach_the_context(env, fn):
    """What is optional or empty is no fault: NULL uright / taken / centres, no queries, and no trains over an empty
    grid all get to the context, still without a write."""
    args_of, reached = FORMS[fn]
    empty = dict(off=np.zeros(CELLS + 1, np.int32), idx=None)
    if fn == "orb_search_by_projection":
        variants = [dict(ur=None), dict(taken=None), dict(nq=0, q=None, qdesc=None), dict(max_dist=0),
                    dict(max_dist=256, mode=1), dict(nt=0, tdesc=None, kps=None, out=False, **empty)]
    else:
        variants = [dict(cen=None), dict(n1=0, desc1=None, kps1=None), dict(window=NAN),
                    dict(n2=0, desc2=None, kps2=None, **empty)]
    for kw in variants:
        assert _call(env, fn, args_of, kw) == (ORB_ERR_ARG, reached), (fn, sorted(kw))
