"""GPU: orb_kfdb_query (k_kfdb_query) and both detect_* calls of orbgpu.KeyFrameDatabase against the restatement
(tests/kfdb_ref.py) on the planted scripts of tests/kfdb_cases.py: ids and their order, common-word counts, the doubles
byte for byte (-0.0 included) and the candidate lists.  What each script plants is checked, without a GPU, by
tests/test_kfdb_ref.py."""
import ctypes

import numpy as np
import pytest

import kfdb_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(orbgpu_mod):
    return orbgpu_mod.ORBmatcher(0.7, True)    # the context every database here shares


@pytest.fixture(scope="module")
def lds(orbgpu_mod):
    return orbgpu_mod._lib.lib().orb_kfdb_query_lds_words()


def _bytes(xs):
    return np.asarray(xs, np.float64).tobytes()


def run_gpu(orbgpu_mod, ctx, script):
    """The script on a fresh orbgpu.KeyFrameDatabase: one result per operation, shaped as kfdb_cases.run_ref's."""
    db = orbgpu_mod.KeyFrameDatabase(ctx)
    covis, out = {}, []
    nb = lambda i: covis.get(i, [])
    try:
        for op in script:
            res = None
            if op[0] == "add":
                res = db.add(op[1])
            elif op[0] == "covis":
                covis[op[1]] = list(op[2])
            elif op[0] == "erase":
                db.erase(op[1])
            elif op[0] == "clear":
                db.clear()
            elif op[0] == "query":
                ids, common, score, xs = db.query(op[1], None, op[2])
                res = {"ids": ids.tolist(), "common": common.tolist(), "score": score.copy(),
                       "excl_score": [None if np.isnan(x) else float(x) for x in xs]}
            elif op[0] == "reloc":
                res = {"ids": db.detect_relocalization_candidates(op[1], None, nb).tolist()}
            elif op[0] == "loop":
                res = {"ids": db.detect_loop_candidates(op[1], None, op[2], op[3], nb).tolist()}
            elif op[0] == "score":
                res = orbgpu_mod.bow_score(op[1], None, op[2], None)
            out.append(res)
        out.append(len(db))
    finally:
        db.close()
    return out


def check(script, got, want):
    nq = 0
    for k, (op, g, w) in enumerate(zip(script, got, want)):
        where = "operation %d %s" % (k, op[0])
        if op[0] == "add":
            assert g == w, where
        elif op[0] == "query":
            assert g["ids"] == w["ids"], where
            assert g["common"] == w["common"], where
            assert _bytes(g["score"]) == _bytes(w["score"]), where      # the doubles, not the floats
            assert len(g["excl_score"]) == len(w["excl_score"]), where
            for a, b in zip(g["excl_score"], w["excl_score"]):
                assert (a is None and b is None) or _bytes([a]) == _bytes([b]), where
            nq += 1
        elif op[0] in ("reloc", "loop"):
            assert g["ids"] == w["ids"], where
        elif op[0] == "score":
            assert _bytes([g]) == _bytes([w]), where
    return nq


@pytest.mark.parametrize("name", ["loop", "reloc", "order", "mutation", "cut5", "cut10", "cut13"])
def test_script_equals_the_restatement(orbgpu_mod, matcher, lds, name):
    script = kc.all_scripts(lds)[name]
    want = kc.run_ref(script)
    got = run_gpu(orbgpu_mod, matcher, script)
    check(script, got, want)
    live = set()
    for op, r in zip(script, want):
        if op[0] == "add":
            live.add(r)
        elif op[0] == "erase":
            live.discard(op[1])
        elif op[0] == "clear":
            live.clear()
    assert got[-1] == len(live)


def test_lengths_and_word_positions(orbgpu_mod, matcher, lds):
    """Keyframes of 0, 1, 63, 64, 65, 128 and 200 words against queries of 0, 1, 64, lds - 1, lds and lds + 1 words:
    both kernel forms (query in LDS, query in global memory) on either side of the staging capacity."""
    script = kc.lengths_script(lds)
    assert check(script, run_gpu(orbgpu_mod, matcher, script), kc.run_ref(script)) == 6


def test_summation_order_is_the_references(orbgpu_mod, matcher):
    q, kf = kc.order_pair()
    db = orbgpu_mod.KeyFrameDatabase(matcher)
    try:
        db.add(kf)
        ids, common, score, _ = db.query(q)
        assert ids.tolist() == [0] and common.tolist() == [41]
        assert score.tobytes() == np.array([0.5]).tobytes()    # -1 then forty -2^-53, one at a time: exactly -1
    finally:
        db.close()


def test_two_handles_on_one_context(orbgpu_mod, matcher):
    s1, s2 = kc.loop_script(), kc.reloc_script()
    w1, w2 = kc.run_ref(s1), kc.run_ref(s2)
    a, b = orbgpu_mod.KeyFrameDatabase(matcher), orbgpu_mod.KeyFrameDatabase(matcher)
    try:
        for op in s1:
            if op[0] == "add":
                a.add(op[1])
        for op in s2:
            if op[0] == "add":
                b.add(op[1])
        a.erase(kc.L_G)
        qa, qb = s1[-2][1], s2[-1][1]
        for _ in range(2):    # interleaved, back to back
            ia, ca, sa, xa = a.query(qa, None, s1[-2][2])
            ib, cb, sb, _ = b.query(qb)
            assert ia.tolist() == w1[-2]["ids"] and ca.tolist() == w1[-2]["common"]
            assert sa.tobytes() == _bytes(w1[-2]["score"])
            assert ib.tolist() == [kc.R_P, kc.R_N, kc.R_R] and cb.tolist() == [10, 3, 10]
            assert xa[:2].tobytes() == _bytes([0.75, -0.0]) and np.isnan(xa[2])
        assert len(a) == 9 and len(b) == 3
    finally:
        a.close()
        b.close()
    assert w2[-1]["ids"] == [kc.R_P]


def test_output_contract_and_argument_checks(orbgpu_mod, matcher):
    L = orbgpu_mod._lib.lib()
    ctx = matcher._ctx.h
    script = kc.loop_script()
    want = kc.run_ref(script)[-2]
    db = orbgpu_mod.KeyFrameDatabase(matcher)
    try:
        for op in script:
            if op[0] == "add":
                db.add(op[1])
        db.erase(kc.L_G)
        w = np.array(sorted(script[-2][1]), np.int32)
        v = np.ones(len(w), np.float64)
        ex = np.array(script[-2][2], np.int32)
        nwant = len(want["ids"])

        def query(cap, excl=ex, words=w, vals=v):
            ids, com = np.full(16, -7, np.int32), np.full(16, -7, np.int32)
            sc, xs = np.full(16, -7.0), np.full(4, -7.0)
            n = ctypes.c_int(-7)
            st = L.orb_kfdb_query(ctx, db.h, len(words), words.ctypes.data, vals.ctypes.data, len(excl),
                                  excl.ctypes.data, xs.ctypes.data, cap, ids.ctypes.data, com.ctypes.data,
                                  sc.ctypes.data, ctypes.byref(n))
            return st, n.value, ids, com, sc, xs

        st, n, ids, com, sc, xs = query(nwant - 1)
        assert st == -3 and n == nwant                                        # ORB_ERR_CAPACITY, *n set
        assert (ids == -7).all() and (com == -7).all() and (sc == -7).all() and (xs == -7).all()
        st, n, ids, com, sc, xs = query(nwant)
        assert st == 0 and n == nwant and ids[:n].tolist() == want["ids"] and com[:n].tolist() == want["common"]
        assert sc[:n].tobytes() == _bytes(want["score"])
        assert (ids[n:] == -7).all() and (com[n:] == -7).all() and (sc[n:] == -7).all()    # nothing past n
        assert xs[:2].tobytes() == _bytes([0.75, -0.0]) and xs[2] == -7 and xs[3] == -7       # erased: untouched
        # ORB_ERR_ARG before any GPU work
        assert query(16, np.array([10], np.int32))[0] == -1                    # an id never issued
        assert query(16, np.array([-1], np.int32))[0] == -1
        assert query(16, ex, np.array([3, 3], np.int32), np.ones(2))[0] == -1
        assert query(16, ex, np.array([3, 4], np.int32), np.array([1.0, np.inf]))[0] == -1
        assert query(-1)[0] == -1
        assert L.orb_kfdb_erase(db.h, kc.L_G) == -1 and L.orb_kfdb_erase(db.h, 10) == -1     # erased / unknown
        assert L.orb_kfdb_erase(db.h, -1) == -1
        nid = ctypes.c_int(-7)
        assert L.orb_kfdb_add(ctx, db.h, 2, np.array([5, 5], np.int32).ctypes.data, np.ones(2).ctypes.data,
                              ctypes.byref(nid)) == -1 and nid.value == -7
        assert len(db) == 9
        # an empty query and an empty database: ORB_OK, *n = 0
        st, n, *_ = query(16, ex, np.zeros(0, np.int32), np.zeros(0))
        assert (st, n) == (0, 0)
        db.clear()
        st, n, ids, com, sc, xs = query(16)
        assert (st, n) == (0, 0) and (xs == -7).all() and len(db) == 0
        assert db.add({1: 0.5}) == 10                                          # ids keep counting
    finally:
        db.close()
