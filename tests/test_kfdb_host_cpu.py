"""CPU, no device: the keyframe-database symbols exist with the header's arity; orb_bow_score and orb_kfdb_candidates
(its call without a handle) equal the restatement; the argument checks that need no context return ORB_ERR_ARG."""
import ctypes
import struct

import numpy as np

import kfdb_cases as kc
import kfdb_ref as kr
from test_resident_frame_abi_cpu import _header_arity

NEW = ["orb_kfdb_create", "orb_kfdb_destroy", "orb_kfdb_add", "orb_kfdb_erase", "orb_kfdb_clear", "orb_kfdb_size",
       "orb_kfdb_query", "orb_kfdb_candidates", "orb_bow_score", "orb_kfdb_query_lds_words"]
RELOC, LOOP = 0, 1


def _lib():
    from orbgpu import _lib
    return _lib


def _arrays(bow):
    w = np.array(sorted(bow), np.int32)
    v = np.array([bow[int(x)] for x in w], np.float64)
    return w, v


def _score(b1, b2):
    L = _lib().lib()
    (w1, v1), (w2, v2) = _arrays(b1), _arrays(b2)
    out = ctypes.c_double(7.0)
    assert L.orb_bow_score(len(w1), w1.ctypes.data, v1.ctypes.data, len(w2), w2.ctypes.data, v2.ctypes.data,
                           ctypes.byref(out)) == 0
    return out.value


def candidates(mode, lst, covis, min_score=0.0, db=None):
    """orb_kfdb_candidates on a sharing list {"ids", "common", "score"} -> (candidate ids, the ids nb was called for)."""
    lib = _lib()
    ids, common = np.array(lst["ids"], np.int32), np.array(lst["common"], np.int32)
    score = np.array(lst["score"], np.float64)
    out = np.full(len(ids) + 1, -7, np.int32)
    nc = ctypes.c_int(-7)
    asked = []

    def nb(_user, kf, dst, cap):
        assert cap == 10
        asked.append(kf)
        got = covis.get(kf, [])[:cap]
        for i, x in enumerate(got):
            dst[i] = x
        return len(got)

    st = lib.lib().orb_kfdb_candidates(db, mode, float(min_score), len(ids), ids.ctypes.data, common.ctypes.data,
                                       score.ctypes.data, lib.KfdbNeighboursFn(nb), None, out.ctypes.data,
                                       ctypes.byref(nc))
    assert st == 0, lib.lib().orb_last_error()
    assert (out[nc.value:] == -7).all()
    return out[:nc.value].tolist(), asked


def with_lists(script):
    """The script with a ("query", bow, connected) in front of every Detect* operation: the list that call works on."""
    out = []
    for op in script:
        if op[0] == "reloc":
            out.append(("query", op[1], []))
        elif op[0] == "loop":
            out.append(("query", op[1], list(op[2])))
        out.append(op)
    return out


def test_symbols_exist_with_the_headers_arity():
    lib = _lib()
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert len(lib.SIGNATURES[name][1]) == _header_arity(name), name
    assert lib.lib().orb_abi_version() == 2    # additions only
    assert lib.lib().orb_kfdb_query_lds_words() >= 64
    import orbgpu
    assert (orbgpu.KFDB_RELOC, orbgpu.KFDB_LOOP) == (RELOC, LOOP)
    for name in ("add", "erase", "clear", "__len__", "query", "detect_relocalization_candidates",
                 "detect_loop_candidates"):
        assert hasattr(orbgpu.KeyFrameDatabase, name)


def test_bow_score_equals_the_restatement_byte_for_byte():
    import orbgpu
    ran = 0
    for script in kc.all_scripts(_lib().lib().orb_kfdb_query_lds_words()).values():
        adds = [op[1] for op in script if op[0] == "add"]
        for op in script:
            pairs = []
            if op[0] == "score":
                pairs = [(op[1], op[2])]
            elif op[0] == "query":
                pairs = [(op[1], k) for k in adds[:12]]
            for a, b in pairs:
                want = kr.l1_score(a, b)
                assert struct.pack("<d", _score(a, b)) == struct.pack("<d", want)
                ran += 1
    assert ran > 100
    q, kf = kc.order_pair()
    assert _score(q, kf) == 0.5                                    # the sequential order, exactly
    assert struct.pack("<d", _score({1: 0.5}, {2: 0.5})) == struct.pack("<d", -0.0)
    assert struct.pack("<d", _score({}, {})) == struct.pack("<d", -0.0)
    assert orbgpu.bow_score(q, None, kf, None) == 0.5
    assert orbgpu.bow_score([2, 5, 9], [0.5, 0.25, 0.25], [2, 7, 9], [0.25, 0.5, 0.25]) == 0.5


def test_candidates_equal_the_restatement_in_both_modes():
    lds = _lib().lib().orb_kfdb_query_lds_words()
    nloop = nreloc = 0
    for name, script in kc.all_scripts(lds).items():
        s = with_lists(script)
        res = kc.run_ref(s)
        covis = {}
        seen_reloc = False
        for k, op in enumerate(s):
            if op[0] == "covis":
                covis[op[1]] = list(op[2])
            if op[0] == "loop":
                got, asked = candidates(LOOP, res[k - 1], covis, op[3])
                assert got == res[k]["ids"], name
                assert asked == res[k]["trace"]["kept"], name          # nb only for lScoreAndMatch, in order
                nloop += 1
            # without a handle every mRelocScore starts at 0.0f: the first relocalisation query of a script
            if op[0] == "reloc" and not seen_reloc:
                seen_reloc = True
                got, asked = candidates(RELOC, res[k - 1], covis)
                assert got == res[k]["ids"], name
                assert asked == res[k]["trace"]["kept"], name
                nreloc += 1
    assert nloop >= 5 and nreloc >= 6


def test_candidates_on_hand_made_lists():
    # loop: 10 in common is the maximum -> minCommonWords 8
    lst = {"ids": [4, 9, 2, 7], "common": [10, 9, 8, 9], "score": [0.5, 0.25, 0.9, 0.125]}
    # 2 is not scored (8 is not > 8) whatever its score; 7 is below min_score but counts for 9
    assert candidates(LOOP, lst, {9: [7, 2, 4]}, 0.25) == ([4], [4, 9])          # 9: 0.25 + 0.125 + 0.5 = 0.875 -> best 4
    assert candidates(LOOP, lst, {}, 0.25) == ([4], [4, 9])                      # 0.25 < 0.75 * 0.5
    assert candidates(LOOP, lst, {}, 0.95) == ([], [])                           # nothing reaches min_score
    # relocalisation: every scored entry is kept; 2 is listed and unscored: it contributes 0.0f, 7 its own score
    # 9: 0.25 + 0 + 0.125 = 0.375, exactly 0.75f * 0.5: dropped
    assert candidates(RELOC, lst, {9: [2, 7]}) == ([4], [4, 9, 7])
    assert candidates(RELOC, lst, {9: [2, 7, 4]}) == ([4], [4, 9, 7])            # 9: 0.875, best keyframe 4; 4 alone below
    assert candidates(RELOC, {"ids": [], "common": [], "score": []}, {}) == ([], [])
    # float accumulation: 0.1f + 0.2f + 0.3f in float, against 0.75f of it
    a, b, c = (float(np.float32(x)) for x in (0.1, 0.2, 0.3))
    acc = np.float32(np.float32(np.float32(a) + np.float32(b)) + np.float32(c))
    edge = float(np.float32(0.75) * acc)    # a second entry exactly on 0.75f * best is dropped, one ulp above is kept
    up = float(np.nextafter(np.float32(edge), np.float32(1)))
    lst = {"ids": [0, 1, 2, 3, 4], "common": [5, 5, 5, 5, 5], "score": [a, b, c, edge, up]}
    got, _ = candidates(RELOC, lst, {0: [1, 2]})
    assert got == [2, 4]    # entry 0 accumulates to acc with best 2; 1, 2 alone are below; 3 on the edge; 4 above


def test_context_free_argument_checks():
    lib = _lib()
    L = lib.lib()
    w = np.array([1, 5, 9], np.int32)
    v = np.array([0.5, 0.25, 0.25], np.float64)
    out = ctypes.c_double(7.0)
    n = ctypes.c_int(7)
    h = ctypes.c_void_p(0xdead)
    ids = np.full(4, 7, np.int32)
    sc = np.full(4, 7.0, np.float64)

    def score(n1, w1, v1, outp=ctypes.byref(out)):
        return L.orb_bow_score(n1, None if w1 is None else w1.ctypes.data, None if v1 is None else v1.ctypes.data,
                               len(w), w.ctypes.data, v.ctypes.data, outp)

    assert score(3, w, v) == 0
    out.value = 7.0
    assert score(3, w, v, None) == -1
    assert score(-1, w, v) == -1
    assert score(3, None, v) == -1
    assert score(3, np.array([1, 1, 9], np.int32), v) == -1                      # not strictly ascending
    assert score(3, np.array([5, 1, 9], np.int32), v) == -1
    assert score(3, np.array([-1, 1, 9], np.int32), v) == -1                     # negative
    assert score(3, w, np.array([0.5, np.nan, 0.25])) == -1
    assert score(3, w, np.array([0.5, 0.25, np.inf])) == -1
    assert L.orb_last_error().decode() == "orb_bow_score: value not finite" and out.value == 7.0
    # the database entry points: a NULL handle, a NULL context
    assert L.orb_kfdb_create(None, ctypes.byref(h)) == -1 and h.value == 0xdead
    assert L.orb_kfdb_create(None, None) == -1
    assert L.orb_kfdb_add(None, None, 3, w.ctypes.data, v.ctypes.data, ctypes.byref(n)) == -1
    assert L.orb_kfdb_erase(None, 0) == -1 and L.orb_kfdb_clear(None) == -1 and L.orb_kfdb_size(None) == 0
    assert L.orb_kfdb_query(None, None, 3, w.ctypes.data, v.ctypes.data, 0, None, None, 4, ids.ctypes.data,
                            ids.ctypes.data, sc.ctypes.data, ctypes.byref(n)) == -1
    L.orb_kfdb_destroy(None)
    # orb_kfdb_candidates
    nb = lib.KfdbNeighboursFn(lambda u, i, o, c: 0)
    bad = lib.KfdbNeighboursFn(lambda u, i, o, c: 11)
    one, com = np.array([3], np.int32), np.array([2], np.int32)

    def cand(mode, cnt, idp, comp, fn, ncp=ctypes.byref(n)):
        return L.orb_kfdb_candidates(None, mode, 0.0, cnt, idp.ctypes.data, comp.ctypes.data, sc.ctypes.data, fn, None,
                                     ids.ctypes.data, ncp)

    assert cand(RELOC, 1, one, com, nb) == 0 and n.value == 1 and ids[0] == 3
    n.value, ids[0] = 7, 7
    assert cand(2, 1, one, com, nb) == -1 and L.orb_last_error().decode() == "orb_kfdb_candidates: unknown mode"
    assert cand(RELOC, -1, one, com, nb) == -1
    assert cand(RELOC, 1, one, com, nb, None) == -1
    assert cand(RELOC, 1, np.array([-3], np.int32), com, nb) == -1
    assert cand(RELOC, 1, one, np.array([0], np.int32), nb) == -1
    assert cand(RELOC, 2, np.array([3, 3], np.int32), np.array([2, 2], np.int32), nb) == -1
    assert cand(LOOP, 1, one, com, bad) == -1
    assert n.value in (7, 0) and ids[0] == 7
