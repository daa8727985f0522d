"""Planted cases of the keyframe-database tests: scripts of database operations, built without a GPU and without an
unseeded random draw, run through the restatement (kfdb_ref) for the expected values.

A script is a list of operations on one database:
    ("add", bow)                               bow = {word: value}; the keyframe's id is its add sequence number
    ("covis", id, [ids])                       GetBestCovisibilityKeyFrames of keyframe id, best first
    ("erase", id) / ("clear",)
    ("query", bow, [excluded ids])             the sharing list with every entry scored (orb_kfdb_query)
    ("reloc", bow)                             DetectRelocalizationCandidates
    ("loop", bow, [connected ids], min_score)  DetectLoopCandidates
    ("score", bow1, bow2)                      ORBVocabulary::score
run_ref(script) returns one result per operation (None for those that return nothing).

Scores are planted exactly: with every query value 1.0 and keyframe values 0 < b <= 1, the term of a common word is
|1 - b| - 1 - b = -2b, so the score is the sum of the keyframe's values on the common words; those are dyadic, so every
partial sum is exact in any order and the float cast is exact."""
import math

import numpy as np

import kfdb_ref

WORD_MAX = 2 ** 31 - 1


def planted_kf(words, score):
    """A keyframe BowVector on `words` whose score against an all-ones query containing them is exactly `score`."""
    words = list(words)
    small = 2.0 ** -10
    bow = {w: small for w in words}
    bow[words[0]] = score - small * (len(words) - 1)
    assert bow[words[0]] > 0
    return bow


# ------------------------------------------------------------------ loop form ------------------------------------
LOOP_MIN_SCORE = 0.25
# keyframe ids of loop_script(), by role
L_A, L_B, L_C, L_D, L_E, L_F, L_G, L_H, L_I, L_J = range(10)


def loop_query():
    return {w: 1.0 for w in range(12)}    # maxCommonWords 12 -> minCommonWords 9: scored iff 10 or more in common


def loop_script():
    r = range
    return [
        ("add", planted_kf(r(2, 12), 0.5)),       # A: first common word is the query's third: listed last, added first
        ("add", planted_kf(r(0, 10), 0.25)),      # B: si == minScore, kept
        ("add", planted_kf(r(0, 10), 0.125)),     # C: scored, below minScore: not a candidate, counts as a neighbour
        ("add", planted_kf(r(0, 9), 0.5)),        # D: exactly minCommonWords in common: not scored, does not count
        ("add", planted_kf(r(0, 12), 0.75)),      # E: connected: excluded, does not count as a neighbour
        ("add", {w: 0.5 for w in r(100, 106)}),   # F: connected, shares no word: excl_score -0.0
        ("add", planted_kf(r(0, 12), 0.625)),     # G: connected, erased before the query: ignored
        ("add", planted_kf(r(1, 11), 0.375)),     # H: acc 0.375, dropped
        ("add", planted_kf(r(0, 10), 0.5625)),    # I: acc == 0.75f * best exactly: dropped
        ("add", planted_kf(r(0, 12), 0.6875)),    # J: 12 in common (the maximum); kept
        ("covis", L_A, [L_C, L_D, L_E, L_G]),     # A: 0.5 + C's 0.125 = 0.625, best stays A
        ("covis", L_B, [L_A]),                    # B: 0.25 + 0.5 = 0.75 (the best), best keyframe A: A returned once
        ("erase", L_G),
        ("query", loop_query(), [L_E, L_F, L_G]),
        ("loop", loop_query(), [L_E, L_F, L_G], LOOP_MIN_SCORE),
    ]


# ------------------------------------------------------------------ relocalisation form ---------------------------
R_P, R_N, R_R = range(3)


def reloc_script():
    q1 = {w: 1.0 for w in range(10)}
    q2 = {w: 1.0 for w in range(20, 30)}
    n = planted_kf(range(0, 3), 0.125)
    n.update(planted_kf(range(20, 30), 0.25))
    return [
        ("add", planted_kf(range(0, 10), 0.5)),      # P
        ("add", n),                                  # N: 3 of q1's words (below the cut), all of q2's
        ("add", planted_kf(range(0, 10), 0.4375)),   # R
        ("covis", R_P, [R_N]),
        ("reloc", q1),    # N is listed, never scored: contributes 0.0f; P 0.5, R 0.4375 > 0.375: [P, R]
        ("reloc", q2),    # scores N: mRelocScore 0.25
        ("reloc", q1),    # N contributes 0.25: P 0.75, R 0.4375 < 0.5625: [P]
    ]


# ------------------------------------------------------------------ the cut -----------------------------------------
def cut_script(max_common):
    """A keyframe with max_common words in common, one with exactly minCommonWords and one with one more."""
    mc = kfdb_ref.min_common_words(max_common)
    q = {w: 1.0 for w in range(max_common)}
    return [
        ("add", planted_kf(range(max_common), 0.5)),
        ("add", planted_kf(range(mc), 0.5)),         # words == minCommonWords: not scored
        ("add", planted_kf(range(mc + 1), 0.5)),     # one above: scored
        ("query", q, []),
        ("reloc", q),
        ("loop", q, [], 0.0),
    ]


# ------------------------------------------------------------------ summation order ---------------------------------
def order_pair():
    """(query, keyframe): the terms are -1 followed by forty of -2^-53, the common words at the keyframe's even places
    0, 2, .., 80 (two 64-word chunks).  Added in word order every partial sum rounds back to -1 (ties to even): the
    score is exactly 0.5.  Any other order of the same terms is not."""
    q = {0: 0.5}
    q.update({10 * k: 2.0 ** -54 for k in range(1, 41)})
    kf = dict(q)
    kf.update({10 * k + 5: 0.25 for k in range(40)})
    return q, kf


def order_terms():
    q, kf = order_pair()
    return [math.fabs(q[w] - kf[w]) - math.fabs(q[w]) - math.fabs(kf[w]) for w in sorted(q)]


def negative_pair():
    rng = np.random.default_rng(77)
    words = sorted(int(w) for w in rng.choice(4000, 150, replace=False))
    q = {w: float(v) for w, v in zip(words[:100], rng.standard_normal(100))}
    kf = {w: float(v) for w, v in zip(words[50:], rng.standard_normal(100))}
    return q, kf


def order_script():
    q, kf = order_pair()
    nq, nkf = negative_pair()
    return [("add", kf), ("add", nkf), ("query", q, []), ("query", nq, []), ("score", q, kf), ("score", nq, nkf),
            ("score", kf, q), ("score", q, {}), ("score", {1: 0.5}, {2: 0.5}), ("score", {3: 0.25, 9: 0.75}, {3: 0.25, 9: 0.75})]


# ------------------------------------------------------------------ lengths and positions ---------------------------
KF_LENGTHS = (0, 1, 63, 64, 65, 128, 200)


def _rand_bow(rng, words):
    v = rng.random(len(words)) + 0.01
    v /= v.sum()
    return {int(w): float(x) for w, x in zip(words, v)}


def lengths_queries(lds):
    """Queries of 0, 1, 64, lds - 1, lds and lds + 1 words.  The 64-word one is the core: word ids 0, 999,999 and
    2^31 - 1, 2500 and 2600, and 59 drawn from [1000, 3000); the long ones add filler words nothing else holds."""
    rng = np.random.default_rng(5)
    pool = [int(w) for w in rng.permutation(np.arange(1000, 3000)) if int(w) not in (2500, 2600)]
    core = sorted([0, 999_999, WORD_MAX, 2500, 2600] + pool[:59])
    out = [{}, _rand_bow(rng, [0]), _rand_bow(rng, core)]
    for n in (lds - 1, lds, lds + 1):
        filler = list(range(2_000_000, 2_000_000 + 2 * (n - 64), 2))
        out.append(_rand_bow(rng, sorted(core + filler)))
    assert [len(q) for q in out] == [0, 1, 64, lds - 1, lds, lds + 1]
    return out


def lengths_script(lds):
    rng = np.random.default_rng(6)
    qs = lengths_queries(lds)
    core = sorted(qs[2])
    draw = lambda n: sorted(int(w) for w in rng.choice(np.arange(1000, 3000), n, replace=False))
    kfs = [
        {},                                                    # 0 words
        _rand_bow(rng, [0]),                                   # 1 word: word id 0, the first word of both vectors
        _rand_bow(rng, draw(63)),
        _rand_bow(rng, core),                                  # 64: every word in common
        _rand_bow(rng, list(range(1, 64)) + [2500, 2600]),     # 65: common at places 63 and 64, across the chunk edge
        _rand_bow(rng, draw(128)),
        _rand_bow(rng, draw(200)),
        _rand_bow(rng, list(range(5000, 5010))),               # no word in common
        _rand_bow(rng, list(range(5100, 5110)) + [WORD_MAX]),  # only its last word (2^31 - 1), the query's last
        _rand_bow(rng, [999_999, 1_500_000]),                  # word 999,999
        _rand_bow(rng, [2_000_000 + 2 * (lds - 64)]),          # a filler word only the lds + 1 query holds: its last but one
    ]
    assert tuple(len(k) for k in kfs[:7]) == KF_LENGTHS
    script = [("add", k) for k in kfs]
    for q in qs:
        script += [("query", q, []), ("reloc", q)]
    return script


# ------------------------------------------------------------------ mutation ----------------------------------------
def mutation_script():
    """30 keyframes of 100 words from a 600-word space (3,000 words: the 1,024-word pool doubles twice), erasures of
    the first, a middle and the last entry, erasures past the compaction point, clear and add again."""
    rng = np.random.default_rng(9)
    bow = lambda n=100: _rand_bow(rng, sorted(int(w) for w in rng.choice(600, n, replace=False)))
    q1, q2 = bow(80), bow(120)
    s = [("add", bow()) for _ in range(30)]
    s += [("covis", i, [(i + 1) % 30, (i + 7) % 30, (i + 13) % 30]) for i in range(30)]
    s += [("query", q1, []), ("query", q2, [3, 4]), ("reloc", q1)]             # two queries back to back
    s += [("erase", 0), ("erase", 14), ("erase", 29), ("query", q1, [0, 5]), ("reloc", q2)]
    s += [("erase", i) for i in range(1, 14)] + [("erase", i) for i in range(15, 20)]   # 21 of 30 dead: compaction
    s += [("query", q1, []), ("add", bow()), ("query", q2, [30]), ("loop", q1, [22, 23], 0.01)]
    s += [("clear",), ("query", q1, []), ("add", bow()), ("add", bow(7)), ("query", q1, [2]), ("reloc", q1)]
    return s


# ------------------------------------------------------------------ the restatement's answers -----------------------
def run_ref(script):
    db = kfdb_ref.KeyFrameDatabase()
    kfs, live, covis = [], set(), {}
    out = []

    def wire():
        for k in kfs:
            k.best_covisibles = [kfs[i] for i in covis.get(k.mnId, []) if i < len(kfs)]

    for op in script:
        res = None
        if op[0] == "add":
            k = kfdb_ref.KeyFrame(len(kfs), op[1])
            kfs.append(k)
            live.add(k.mnId)
            db.add(k)
            res = k.mnId
        elif op[0] == "covis":
            covis[op[1]] = list(op[2])
        elif op[0] == "erase":
            db.erase(kfs[op[1]])
            live.discard(op[1])
        elif op[0] == "clear":
            db.clear()
            live.clear()
        elif op[0] == "query":
            lst = db.sharing(op[1], [kfs[i] for i in op[2]])
            excl = [kfdb_ref.l1_score(op[1], kfs[i].mBowVec) if i in live else None for i in op[2]]
            res = {"ids": [k.mnId for k, _, _ in lst], "common": [c for _, c, _ in lst],
                   "score": [s for _, _, s in lst], "excl_score": excl}
        elif op[0] == "reloc":
            wire()
            got = db.DetectRelocalizationCandidates(kfdb_ref.Frame(kfdb_ref.next_query_id(), op[1]))
            res = {"ids": [k.mnId for k in got], "trace": db.last_trace}
        elif op[0] == "loop":
            wire()
            q = kfdb_ref.KeyFrame(kfdb_ref.next_query_id(), op[1])
            q.connected = [kfs[i] for i in op[2]]
            got = db.DetectLoopCandidates(q, op[3])
            res = {"ids": [k.mnId for k in got], "trace": db.last_trace}
        elif op[0] == "score":
            res = kfdb_ref.l1_score(op[1], op[2])
        else:
            raise ValueError(op[0])
        out.append(res)
    return out


def all_scripts(lds):
    s = {"loop": loop_script(), "reloc": reloc_script(), "order": order_script(), "lengths": lengths_script(lds),
         "mutation": mutation_script()}
    for m in (5, 10, 13):
        s["cut%d" % m] = cut_script(m)
    return s


# ------------------------------------------------------------------ a script as text (the C++ adapter's driver) -----
def _bow_text(bow):
    return " ".join([str(len(bow))] + ["%d %s" % (w, float(bow[w]).hex()) for w in sorted(bow)])


def to_text(script):
    """One operation per line; doubles as C99 hex floats (exact)."""
    lines = []
    for op in script:
        if op[0] == "add":
            lines.append("add " + _bow_text(op[1]))
        elif op[0] == "covis":
            lines.append("covis %d %d %s" % (op[1], len(op[2]), " ".join(map(str, op[2]))))
        elif op[0] == "erase":
            lines.append("erase %d" % op[1])
        elif op[0] == "clear":
            lines.append("clear")
        elif op[0] == "query":
            continue    # (the adapter has no such member)
        elif op[0] == "reloc":
            lines.append("reloc " + _bow_text(op[1]))
        elif op[0] == "loop":
            lines.append("loop %s %d %s %s" % (float(np.float32(op[3])).hex(), len(op[2]), " ".join(map(str, op[2])),
                                               _bow_text(op[1])))
        elif op[0] == "score":
            lines.append("score %s %s" % (_bow_text(op[1]), _bow_text(op[2])))
    return "\n".join(lines) + "\n"
