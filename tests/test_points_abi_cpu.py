"""CPU: the resident map point symbols exist in liborbgpu.so with the header's arity, the ctypes structs have the
header's layout, and every argument check returns ORB_ERR_ARG without a device, before the context (NULL here) is looked
at and with no output written."""
import ctypes
import os
import re

import numpy as np

import frustum_cases as fc
from conftest import ROOT

NEW = ["orb_points_create", "orb_points_write", "orb_points_capacity", "orb_points_destroy", "orb_project_points",
       "orb_project_points_host", "orb_search_local_points", "orb_fuse_search_points"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbgpu.h")).read(), flags=re.S)


def _header_arity(name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else args.count(",") + 1


def _struct_fields(name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S)
    assert m, name
    return re.findall(r"(\w+)\s*(?:\[[^\]]*\])?\s*[;,]", m.group(1))


def test_symbols_exist_with_the_headers_arity():
    from orbgpu import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert len(_lib.SIGNATURES[name][1]) == _header_arity(name), name
    assert _lib.lib().orb_abi_version() == 2   # additions only


def test_structs_have_the_headers_fields(orbgpu_mod):
    from orbgpu import _lib
    assert [f for f, _ in _lib.OrbCamera._fields_] == _struct_fields("orb_camera")
    assert [f for f, _ in _lib.OrbFusePointsTarget._fields_] == _struct_fields("orb_fuse_points_target")
    assert list(orbgpu_mod.POINT_PROJ_DTYPE.names) == _struct_fields("orb_point_proj")
    assert ctypes.sizeof(_lib.OrbCamera) == 42 * 4 and orbgpu_mod.POINT_PROJ_DTYPE.itemsize == 36


def test_points_handle_argument_checks(orbgpu_mod):
    from orbgpu import _lib
    L = _lib.lib()
    err = lambda: L.orb_last_error().decode()
    h = ctypes.c_void_p(0xdead)
    assert L.orb_points_create(None, -1, ctypes.byref(h)) == -1 and err() == "orb_points_create: capacity < 0"
    assert L.orb_points_create(None, 4, None) == -1
    assert L.orb_points_create(None, 4, ctypes.byref(h)) == -1 and err() == "NULL context"
    assert h.value == 0xdead
    # orb_points_write checks its arrays before it touches the handle's device: a handle that is not one is never read
    fake = ctypes.create_string_buffer(64)
    n = 3
    pos, nr = np.ones((n, 3), np.float32), np.ones((n, 3), np.float32)
    lo, hi, d = np.ones(n, np.float32), np.ones(n, np.float32), np.zeros((n, 32), np.uint8)
    P = lambda a: a.ctypes.data

    def write(first=0, cnt=n, pos=pos, nr=nr, lo=lo, hi=hi, d=d, handle=fake):
        return L.orb_points_write(handle, first, cnt, None if pos is None else P(pos), P(nr), P(lo), P(hi),
                                  None if d is None else P(d))

    assert write(handle=None) == -1 and err() == "orb_points_write: NULL handle"
    assert write(first=-1) == -1 and write(cnt=-1) == -1
    assert write(first=2 ** 31 - 2) == -1 and err() == "orb_points_write: slot range beyond INT_MAX"
    assert write(pos=None) == -1 and write(d=None) == -1 and err() == "orb_points_write: NULL arrays with n > 0"
    for arr, name in ((pos, "position or normal"), (nr, "position or normal"), (lo, "distance"), (hi, "distance")):
        for bad in (np.nan, np.inf, -np.inf):
            b = arr.copy()
            b.flat[b.size - 1] = bad
            kw = {"pos": pos, "nr": nr, "lo": lo, "hi": hi}
            kw[[k for k, v in kw.items() if v is arr][0]] = b
            assert write(**kw) == -1 and err() == "orb_points_write: %s not finite" % name
    assert L.orb_points_capacity(None) == 0
    L.orb_points_destroy(None)


def test_projection_entry_point_argument_checks(orbgpu_mod):
    from orbgpu import _lib
    L = _lib.lib()
    err = lambda: L.orb_last_error().decode()
    cam = fc.cam_struct(orbgpu_mod, fc.PLANT_CAM)
    ids = np.zeros(4, np.int32)
    out = np.full(4, 7, orbgpu_mod.POINT_PROJ_DTYPE)
    match = np.full(8, 7, np.int32)
    nm = ctypes.c_int(7)
    P = lambda a: a.ctypes.data

    def project(mode=0, cam=cam, limit=0.5, th=1.0, n=4):
        return L.orb_project_points(None, None, mode, ctypes.byref(cam), limit, th, n, P(ids), P(out))

    def local(cam=cam, limit=0.5, th=1.0, n=4):
        return L.orb_search_local_points(None, None, ctypes.byref(cam), limit, th, 0.8, n, P(ids), None, None, 0,
                                         P(match), ctypes.byref(nm), P(out))

    def host(mode=0, cam=cam, limit=0.5, th=1.0, n=1):
        a = np.ones(3, np.float32)
        return L.orb_project_points_host(mode, ctypes.byref(cam), limit, th, n, P(a), P(a), P(a), P(a), P(out))

    assert project(mode=2) == -1 and err() == "orb_project_points: unknown mode"
    assert host(mode=-1) == -1 and err() == "orb_project_points_host: unknown mode"
    assert project() == -1 and err() == "orb_project_points: NULL points handle"
    assert local() == -1 and err() == "orb_search_local_points: NULL points handle"
    assert L.orb_project_points(None, None, 0, None, 0.5, 1.0, 4, P(ids), P(out)) == -1 and err().endswith("camera NULL")
    for call in (project, local, host):
        for th in (np.nan, np.inf, -1.0):
            assert call(th=th) == -1 and err().endswith("th not finite or negative")
        assert call(limit=np.nan) == -1 and err().endswith("view_cos_limit not finite")
        for field in ("fx", "fy", "cx", "cy", "mbf", "min_x", "max_x", "min_y", "max_y"):
            for bad in (np.nan, np.inf):
                c = fc.cam_struct(orbgpu_mod, fc.PLANT_CAM)
                setattr(c, field, bad)
                assert call(cam=c) == -1 and err().endswith("camera field not finite"), field
        for field, size in (("Rcw", 9), ("tcw", 3), ("Ow", 3), ("scale_factors", fc.NLEVELS)):
            for i in (0, size - 1):
                c = fc.cam_struct(orbgpu_mod, fc.PLANT_CAM)
                getattr(c, field)[i] = float("nan")
                assert call(cam=c) == -1 and err().endswith("camera field not finite"), field
        for nlevels in (0, 17, -3):
            c = fc.cam_struct(orbgpu_mod, fc.PLANT_CAM)
            c.nlevels = nlevels
            assert call(cam=c) == -1 and err().endswith("nlevels outside [1, ORBGPU_MAX_LEVELS]")
        for lsf in (0.0, -0.1, np.nan, np.inf):
            c = fc.cam_struct(orbgpu_mod, fc.PLANT_CAM)
            c.log_scale_factor = lsf
            assert call(cam=c) == -1 and err().endswith("log_scale_factor not finite or <= 0")
    assert host(n=-1) == -1
    # a scale factor past nlevels is not read
    c = fc.cam_struct(orbgpu_mod, fc.PLANT_CAM)
    c.scale_factors[15] = float("nan")
    assert host(cam=c) == 0
    # the fused Fuse call: a NULL handle, a negative count, NULL targets
    assert L.orb_fuse_search_points(None, None, 0, None) == -1 and err() == "orb_fuse_search_points: NULL points handle"
    assert (out["verdict"][1:] == 7).all() and (match == 7).all() and nm.value == 7
