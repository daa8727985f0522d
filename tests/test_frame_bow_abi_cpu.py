"""CPU: the BoW-on-the-handle symbols exist in liborbgpu.so with the header's arity, and the argument checks that need
neither a device nor a live handle return ORB_ERR_ARG: a NULL handle, negative counts, nlevels2 out of range, and a
FeatureVector CSR whose own shape is wrong.  The checks that need a handle (one without BoW, a feature index >= n)
are in tests/test_gpu_triangulation_frames.py.  The ABI version stays 2: the additions change no existing layout, and
tests/test_abi_cpu.py pins 2."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

NEW = ["orb_frame_compute_bow", "orb_frame_set_featvec", "orb_frame_has_bow", "orb_frame_bow_read",
       "orb_search_for_triangulation_frames", "orb_search_by_bow_frames_kf_f", "orb_search_by_bow_frames_kf_kf"]


def _header():
    src = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_arity(name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else args.count(",") + 1


def _struct_fields(name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(",")
        out.append(re.findall(r"\w+", names[0])[-1])
        out += [re.findall(r"\w+", x)[-1] for x in names[1:]]
    return out


def test_symbols_exist_with_the_headers_arity():
    from orbgpu import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert len(_lib.SIGNATURES[name][1]) == _header_arity(name), name
    assert _lib.lib().orb_abi_version() == 2   # additions only
    assert [f for f, _ in _lib.OrbTriFramePair._fields_] == _struct_fields("orb_tri_frame_pair")
    assert [f for f, _ in _lib.OrbBowFrameKf._fields_] == _struct_fields("orb_bow_frame_kf")


def test_context_free_argument_checks(orbgpu_mod):
    from orbgpu import _lib
    L = _lib.lib()
    out = np.full(8, 7, np.int32)
    nm = ctypes.c_int(7)
    flags = np.ones(4, np.uint8)
    F12 = np.zeros(9, np.float32)
    lv = np.ones(8, np.float32)

    def err():
        return L.orb_last_error().decode()

    def pair(nlevels2):
        return _lib.OrbTriFramePair(None, flags.ctypes.data, F12.ctypes.data, 0.0, 0.0, lv.ctypes.data, lv.ctypes.data,
                                    nlevels2, out.ctypes.data, 4, ctypes.pointer(nm))

    tri = L.orb_search_for_triangulation_frames
    P = pair(8)
    assert tri(None, 1, 0, None, flags.ctypes.data, -1, ctypes.addressof(P)) == -1
    assert err() == "orb_search_for_triangulation_frames: bad arguments"
    assert tri(None, 1, 0, None, flags.ctypes.data, 1, None) == -1
    for bad in (0, 17, -3):
        Pb = pair(bad)
        assert tri(None, 1, 0, None, flags.ctypes.data, 1, ctypes.addressof(Pb)) == -1
        assert err() == "orb_search_for_triangulation_frames: nlevels2 outside [1, ORBGPU_MAX_LEVELS]"
    assert tri(None, 1, 0, None, flags.ctypes.data, 1, ctypes.addressof(P)) == -1
    assert err() == "orb_search_for_triangulation_frames: NULL frame"
    assert tri(None, 1, 0, None, flags.ctypes.data, 0, None) == -1   # (a NULL frame1 even with nothing to do)

    K = _lib.OrbBowFrameKf(None, flags.ctypes.data, out.ctypes.data, ctypes.pointer(nm))
    kf_f = L.orb_search_by_bow_frames_kf_f
    assert kf_f(None, 0.7, 1, None, -1, ctypes.addressof(K)) == -1
    assert err() == "orb_search_by_bow_frames_kf_f: bad arguments"
    assert kf_f(None, 0.7, 1, None, 1, None) == -1
    assert kf_f(None, 0.7, 1, None, 1, ctypes.addressof(K)) == -1
    assert err() == "orb_search_by_bow_frames_kf_f: NULL frame"
    assert L.orb_search_by_bow_frames_kf_kf(None, 0.7, 1, None, flags.ctypes.data, None, flags.ctypes.data,
                                            out.ctypes.data, ctypes.byref(nm)) == -1
    assert err() == "orb_search_by_bow_frames_kf_kf: NULL frame"

    hs = (ctypes.c_void_p * 2)(None, None)
    cb = L.orb_frame_compute_bow
    assert cb(None, None, 4, -1, hs) == -1 and err() == "orb_frame_compute_bow: nframes < 0"
    assert cb(None, None, 4, 1, None) == -1 and err() == "orb_frame_compute_bow: frames NULL"
    assert cb(None, None, 4, 1, hs) == -1 and err() == "orb_frame_compute_bow: NULL vocabulary"
    assert L.orb_frame_has_bow(None) == 0
    assert L.orb_frame_bow_read(None, None, None, None, ctypes.byref(nm), None, out.ctypes.data, None,
                                ctypes.byref(nm)) == -1
    assert err() == "orb_frame_bow_read: NULL frame"

    # orb_frame_set_featvec: the CSR's own shape is checked before the handle is looked at
    def fv(nodes, off, idx):
        a = [np.array(nodes, np.uint32), np.array(off, np.int32), np.array(idx, np.int32)]
        return _lib.OrbFeatVec(len(nodes), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data), a

    sf = L.orb_frame_set_featvec
    for nodes, off, idx in (([3, 5], [1, 2, 3], [0, 1, 2]),      # offsets do not start at 0
                            ([3, 5], [0, 2, 1], [0, 1, 2]),      # offsets decrease
                            ([5, 3], [0, 1, 2], [0, 1]),         # node ids not ascending
                            ([3, 3], [0, 1, 2], [0, 1]),         # node ids not strictly ascending
                            ([3, 5], [0, 1, 2], [0, -1])):       # a negative index
        s, keep = fv(nodes, off, idx)
        assert sf(None, None, s) == -1
        assert err() == "orb_frame_set_featvec: malformed FeatureVector CSR", (nodes, off, idx)
    s, keep = fv([3, 5], [0, 1, 2], [0, 1])
    assert sf(None, None, s) == -1 and err() == "orb_frame_set_featvec: NULL frame"
    assert (out == 7).all() and nm.value == 7
