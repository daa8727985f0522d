"""CPU: the keyframe-database restatement (tests/kfdb_ref.py) pinned by hand-computed answers, and the planted
decisions of tests/kfdb_cases.py found in its trace."""
import math
import struct

import numpy as np

import kfdb_cases as kc
import kfdb_ref as kr

LDS = 4096    # any capacity serves the builders here; the GPU tests pass the library's


def _bits(x):
    return struct.pack("<d", x)


def test_identical_normalised_vectors_score_one():
    v = {3: 0.25, 9: 0.5, 70: 0.25}
    assert kr.l1_score(v, dict(v)) == 1.0


def test_disjoint_vectors_score_minus_zero():
    s = kr.l1_score({1: 0.5, 5: 0.5}, {2: 0.5, 6: 0.5})
    assert s == 0.0 and math.copysign(1.0, s) == -1.0 and _bits(s) == _bits(-0.0)
    s = kr.l1_score({1: 1.0}, {})
    assert _bits(s) == _bits(-0.0)


def test_three_word_example():
    """v1 = {2: 0.5, 5: 0.25, 9: 0.25}, v2 = {2: 0.25, 7: 0.5, 9: 0.25}.  Common words 2 and 9:
         word 2: |0.5 - 0.25| - 0.5 - 0.25 = -0.5
         word 9: |0.25 - 0.25| - 0.25 - 0.25 = -0.5
       score = -(-0.5 + -0.5) / 2 = 0.5 (= 1 - ||v1 - v2||_1 / 2 = 1 - (0.25 + 0.25 + 0.5 + 0) / 2)."""
    v1, v2 = {2: 0.5, 5: 0.25, 9: 0.25}, {2: 0.25, 7: 0.5, 9: 0.25}
    assert kr.l1_score(v1, v2) == 0.5 and kr.l1_score(v2, v1) == 0.5


def test_the_cut_for_every_max_up_to_300():
    """int(maxCommonWords * 0.8f).  0.8f = 13421773 / 2^24 = 0.8 + 2^-24 / 5 * 1 (0.800000011920929), so the exact
    product is 0.8 n + n * 1.1920929e-8 with n <= 300: an excess below 3.6e-6.  0.8 n = 4n / 5 has fractional part 0,
    0.2, 0.4, 0.6 or 0.8; rounding the product to float moves it by at most half an ulp, 2^-16 = 1.53e-5 below 512; so
    the float lies within 1.9e-5 of 4n / 5 and never below it when 4n / 5 is an integer (the exact product is above the
    integer, which is itself a float, and rounding is monotonic).  Truncation therefore gives floor(4n / 5)."""
    for n in range(1, 301):
        assert kr.min_common_words(n) == (4 * n) // 5, n
    assert [kr.min_common_words(n) for n in (5, 10, 13)] == [4, 8, 10]


def test_order_case_detects_a_wrong_summation_order():
    t = kc.order_terms()
    assert t[0] == -1.0 and t[1:] == [-2.0 ** -53] * 40
    seq = 0.0
    for x in t:
        seq += x
    assert seq == -1.0
    rev = 0.0
    for x in reversed(t):
        rev += x
    tree = list(t)
    while len(tree) > 1:    # pairwise tree, as a butterfly or a tree reduction adds
        tree = [tree[i] + tree[i + 1] if i + 1 < len(tree) else tree[i] for i in range(0, len(tree), 2)]
    assert rev != seq and tree[0] != seq
    q, kf = kc.order_pair()
    assert kr.l1_score(q, kf) == 0.5 and _bits(-rev / 2.0) != _bits(0.5) and _bits(-tree[0] / 2.0) != _bits(0.5)
    # the common words sit at the keyframe's places 0, 2, .., 80: both 64-word chunks
    places = [i for i, w in enumerate(sorted(kf)) if w in q]
    assert places == list(range(0, 81, 2))
    nq, nkf = kc.negative_pair()
    assert min(nq.values()) < 0 and min(nkf.values()) < 0 and len(set(nq) & set(nkf)) == 50


def test_loop_script_plants_every_decision():
    res = kc.run_ref(kc.loop_script())
    query, loop = res[-2], res[-1]
    A, B, C, D, E, F, G, H, I, J = range(10)
    # the later-added keyframes precede A (its first common word is later); equal first words: add order
    assert query["ids"] == [B, C, D, I, J, H, A]
    assert query["common"] == [10, 10, 9, 10, 12, 10, 10]
    assert query["score"] == [0.25, 0.125, 0.5, 0.5625, 0.6875, 0.375, 0.5]
    assert query["excl_score"][0] == 0.75 and struct.pack("<d", query["excl_score"][1]) == _bits(-0.0)
    assert query["excl_score"][2] is None    # erased: left untouched
    tr = loop["trace"]
    assert tr["min_common"] == 9
    assert [i for i, _ in tr["sharing"]] == query["ids"]
    assert [i for i, _ in tr["scored"]] == [B, C, I, J, H, A]            # D sits exactly at minCommonWords
    assert tr["kept"] == [B, I, J, H, A]                                 # si == minScore kept (B), C below it
    assert tr["counted"] == [(B, A), (A, C)]                             # C counts; D (cut), E (excluded), G (erased) do not
    assert tr["acc"] == [(B, 0.75, A), (I, 0.5625, I), (J, 0.6875, J), (H, 0.375, H), (A, 0.625, A)]
    assert tr["retain"] == 0.5625                                        # I sits exactly on it: dropped
    assert loop["ids"] == [A, J]                                         # A once, though two entries name it


def test_reloc_script_plants_the_carried_score():
    r1, r2, r3 = kc.run_ref(kc.reloc_script())[-3:]
    P, N, R = range(3)
    assert r1["trace"]["counted"] == [(P, N, 0.0)] and r1["ids"] == [P, R]
    assert r2["ids"] == [N] and r2["trace"]["scored"] == [(N, 0.25)]
    assert r3["trace"]["counted"] == [(P, N, 0.25)] and r3["trace"]["acc"][0] == (P, 0.75, P) and r3["ids"] == [P]
    assert [i for i, _ in r3["trace"]["scored"]] == [P, R]               # N is listed but below the cut


def test_cut_scripts_plant_the_boundary():
    for m, mc in ((5, 4), (10, 8), (13, 10)):
        res = kc.run_ref(kc.cut_script(m))
        q, reloc, loop = res[-3:]
        assert q["ids"] == [0, 1, 2] and q["common"] == [m, mc, mc + 1]
        for r in (reloc, loop):
            assert r["trace"]["min_common"] == mc and [i for i, _ in r["trace"]["scored"]] == [0, 2]


def test_lengths_and_mutation_scripts_cover_their_cases():
    s = kc.lengths_script(LDS)
    res = kc.run_ref(s)
    adds = [op[1] for op in s if op[0] == "add"]
    assert tuple(len(k) for k in adds[:7]) == kc.KF_LENGTHS
    queries = [(op, r) for op, r in zip(s, res) if op[0] == "query"]
    assert [len(op[1]) for op, _ in queries] == [0, 1, 64, LDS - 1, LDS, LDS + 1]
    assert queries[0][1]["ids"] == [] and queries[1][1]["ids"] == [1, 3]     # word id 0: first word of both vectors
    r64 = queries[2][1]
    assert r64["common"][r64["ids"].index(3)] == 64                       # every word in common
    assert r64["common"][r64["ids"].index(4)] == 2                        # places 63 and 64 of the 65-word keyframe
    assert 7 not in r64["ids"] and r64["common"][r64["ids"].index(8)] == 1 and 9 in r64["ids"]
    assert r64["ids"][-1] == 8                                            # its only common word is the query's last
    assert all(10 not in r["ids"] for _, r in queries[:5]) and 10 in queries[5][1]["ids"]
    for _, r in queries[2:]:
        assert {2, 5, 6} <= set(r["ids"])                                 # the 63-, 128- and 200-word keyframes share words
    m = kc.mutation_script()
    mres = kc.run_ref(m)
    assert sum(len(op[1]) for op in m[:30]) == 3000                       # 1,024 -> 2,048 -> 4,096 words
    ids_after_clear = [r for op, r in zip(m, mres) if op[0] == "add"][-2:]
    assert ids_after_clear == [31, 32]
    last_q = [r for op, r in zip(m, mres) if op[0] == "query"][-1]
    assert last_q["ids"] and set(last_q["ids"]) <= {31, 32} and last_q["excl_score"] == [None]
    first_q = [r for op, r in zip(m, mres) if op[0] == "query"][0]
    assert len(first_q["ids"]) == 30 and first_q["ids"] != sorted(first_q["ids"])


def test_to_text_round_trips_the_doubles():
    txt = kc.to_text(kc.order_script())
    line = [ln for ln in txt.splitlines() if ln.startswith("score")][0].split()
    assert float.fromhex(line[3]) == 0.5 and float.fromhex(line[5]) == 2.0 ** -54
    assert np.float32(kc.LOOP_MIN_SCORE) == 0.25
