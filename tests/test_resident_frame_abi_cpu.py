"""CPU: the resident-frame symbols exist in liborbgpu.so with the header's arity, and the argument checks that need no
context (NULL handle, unknown mode, max_dist out of range, bad grid geometry) return ORB_ERR_ARG without a device."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

NEW = ["orb_frame_create", "orb_frame_create_device", "orb_frame_destroy", "orb_frame_count", "orb_frame_grid_read",
       "orb_search_by_projection_frame", "orb_window_match_frame", "orb_search_by_match_bird_resident",
       "orb_project_best_frames"]


def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else args.count(",") + 1


def test_symbols_exist_with_the_headers_arity():
    from orbgpu import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert len(_lib.SIGNATURES[name][1]) == _header_arity(name), name
    assert _lib.lib().orb_abi_version() == 2   # additions only
    # orb_proj_frame_target: the struct's fields in the header's order
    assert [f for f, _ in _lib.OrbProjFrameTarget._fields_] == ["nq", "q", "qdesc", "frame", "inv_sigma2", "nlevels",
                                                                "best_idx", "best_dist"]


def test_context_free_argument_checks(orbgpu_mod):
    from orbgpu import _lib
    L = _lib.lib()
    nq = 4
    q = np.zeros(nq, orbgpu_mod.PROJ_QUERY_DTYPE)
    q["r"] = 5.0
    qd = np.zeros((nq, 32), np.uint8)
    k = np.zeros(nq, orbgpu_mod.KP_DTYPE)
    out = np.full(8, 7, np.int32)
    nm = ctypes.c_int(7)

    def err():
        return L.orb_last_error().decode()

    def proj(mode, max_dist):
        return L.orb_search_by_projection_frame(None, mode, 0.8, 1, max_dist, nq, q.ctypes.data, qd.ctypes.data, None,
                                                None, 0, out.ctypes.data, ctypes.byref(nm))

    assert proj(0, 100) == -1 and err() == "orb_search_by_projection_frame: NULL frame"
    assert proj(2, 100) == -1 and err() == "orb_search_by_projection_frame: unknown mode"
    assert proj(0, 257) == -1 and err() == "orb_search_by_projection_frame: max_dist outside [0, 256]"
    assert proj(0, -1) == -1
    assert L.orb_window_match_frame(None, 0.8, 1, 0, nq, qd.ctypes.data, k.ctypes.data, None, 10.0, None,
                                    out.ctypes.data, ctypes.byref(nm)) == -1
    assert err() == "orb_window_match_frame: NULL frame"
    xy = np.zeros((nq, 2), np.float32)
    assert L.orb_search_by_match_bird_resident(None, 0.8, 0, 100, 10.0, nq, None, xy.ctypes.data, None, qd.ctypes.data,
                                               None, out.ctypes.data, ctypes.byref(nm)) == -1
    assert err() == "orb_search_by_match_bird_resident: NULL frame"
    assert L.orb_search_by_match_bird_resident(None, 0.8, 0, 300, 10.0, nq, None, xy.ctypes.data, None, qd.ctypes.data,
                                               None, out.ctypes.data, ctypes.byref(nm)) == -1
    assert err() == "orb_search_by_match_bird_resident: max_dist outside [0, 256]"
    T = _lib.OrbProjFrameTarget(nq, q.ctypes.data, qd.ctypes.data, None, None, 0, out.ctypes.data, out.ctypes.data)
    assert L.orb_project_best_frames(None, 0, 1, ctypes.addressof(T)) == -1
    assert err() == "orb_project_best_frames: target 0: NULL frame"
    assert L.orb_project_best_frames(None, 3, 1, ctypes.addressof(T)) == -1
    assert err() == "orb_project_best_frames: unknown gate"
    # the creators: checked before the context (NULL here) is looked at
    h = ctypes.c_void_p(0xdead)
    for fn in (L.orb_frame_create, L.orb_frame_create_device):
        assert fn(None, -1, qd.ctypes.data, k.ctypes.data, None, 0.0, 0.0, 0.1, 0.1, ctypes.byref(h)) == -1
        assert fn(None, nq, None, k.ctypes.data, None, 0.0, 0.0, 0.1, 0.1, ctypes.byref(h)) == -1
        assert fn(None, nq, qd.ctypes.data, k.ctypes.data, None, 0.0, 0.0, 0.0, 0.1, ctypes.byref(h)) == -1
        assert fn(None, nq, qd.ctypes.data, k.ctypes.data, None, float("nan"), 0.0, 0.1, 0.1, ctypes.byref(h)) == -1
        assert fn(None, nq, qd.ctypes.data, k.ctypes.data, None, 0.0, 0.0, 0.1, 0.1, ctypes.byref(h)) == -1
        assert err() == "NULL context"
    kb = k.copy()
    kb["y"][2] = np.inf
    assert L.orb_frame_create(None, nq, qd.ctypes.data, kb.ctypes.data, None, 0.0, 0.0, 0.1, 0.1, ctypes.byref(h)) == -1
    assert err() == "orb_frame_create: keypoint position not finite"
    assert h.value == 0xdead and (out == 7).all() and nm.value == 7
    L.orb_frame_destroy(None)
    assert L.orb_frame_count(None) == 0
