"""The planted-decision cases of k_describe (tests/describe_cases.py) against the oracle, on the CPU: describe_ref
equals the oracle on every frame (keypoints, angles, descriptors, and the blur stage by stage), every planted keypoint
is a keypoint at its planted position, every hand-written expectation holds in the reference trace, the census is
realised except for the items describe_cases.UNREACHED names, and each mutated rule of the reference changes the
output of the cases planted for it."""
import numpy as np
import pytest

import describe_cases as C
import describe_ref as R

_ORACLE = {}


def _oracle_run(oracle_mod, f, flags=0):
    """(keypoints, descriptors, per level (x, y, response) rows, extractor) of a frame, computed once and shared."""
    key = (f.name, flags)
    if key not in _ORACLE:
        o = oracle_mod.OracleExtractor(f.nfeatures, f.scale, f.nlevels, flags=flags)
        k, d = o(f.img)
        lk = [[(int(p["x"]), int(p["y"]), float(p["response"])) for p in o.level_keypoints(l)]
              for l in range(f.nlevels)]
        _ORACLE[key] = (k, d, lk, o)
    return _ORACLE[key]


_REF = {}


def _ref(oracle_mod, f, rules=R.PINNED):
    key = (f.name, rules)
    if key not in _REF:
        _REF[key] = R.extract(f.levels, _oracle_run(oracle_mod, f)[2], f.scale, rules)
    return _REF[key]


def _traces(oracle_mod, f, rules=R.PINNED):
    return {(t.level, t.x, t.y): t for t in _ref(oracle_mod, f, rules)[2]}


FRAMES = C.frames()
IDS = [f.name for f in FRAMES]


def test_restated_tables_and_arithmetic(oracle_mod):
    assert R.UMAX == oracle_mod.OracleExtractor(100).tables()["umax"].tolist()
    for v0 in range(258):
        for v1 in range(258):
            a, b = R.saturate_forms(v0, v1)
            assert a == b, (v0, v1)
    # the array fma against the exact one on rotated pattern points, and on ties of the final rounding
    from kf_projection_ref import fmaf
    rng = np.random.default_rng(5)
    pat = R.pattern_points()
    ang = (rng.random(40) * 360).astype(R.f32)
    s, c = R.sincos((ang * R.FACTOR_PI).astype(R.f32), "glibc")
    for i in range(40):
        j = int(rng.integers(0, 512))
        px, py = pat[j]
        t = R.f32(py * c[i])
        assert R.fma32(px, s[i], t) == fmaf(px, s[i], t), (i, j)
    a, b, c3 = R.f32(1 + 2.0 ** -23), R.f32(1 + 2.0 ** -23), R.f32(2.0 ** -60)
    for cc in (c3, -c3, R.f32(0)):
        assert R.fma32(a, b, cc) == fmaf(a, b, cc)


@pytest.mark.parametrize("f", FRAMES, ids=IDS)
def test_reference_equals_oracle(oracle_mod, f):
    ok, od, lk, o = _oracle_run(oracle_mod, f)
    k, d, tr = _ref(oracle_mod, f)
    assert k.tobytes() == ok.tobytes(), [(t.level, t.x, t.y) for t, a, b in zip(tr, k, ok) if a != b][:5]
    assert np.array_equal(d, od), [(t.level, t.x, t.y) for t, a, b in zip(tr, d, od) if (a != b).any()][:5]
    for t in tr:   # fastAtan2 restated
        assert float(t.angle) == oracle_mod.fast_atan2(float(t.m01), float(t.m10))
    for l, lv in enumerate(f.levels):
        assert np.array_equal(o.level(l), lv), l       # level 1 of the 2 x 2 block frames is the block values
        assert np.array_equal(R.blur(lv), oracle_mod.blur(lv)) and np.array_equal(R.blur(lv), o.blurred(l)), l
        assert np.array_equal(R.blur(lv, R.PINNED._replace(blur="halfup")),
                              oracle_mod.blur(lv, oracle_mod.BLUR_ALL_HALFUP)), l


@pytest.mark.parametrize("flag,rules", [("BLUR_ALL_HALFUP", R.PINNED._replace(blur="halfup")),
                                        ("NO_FMA", R.PINNED._replace(fma=False)),
                                        ("TRIG_CR", R.PINNED._replace(trig="cr"))])
@pytest.mark.parametrize("f", FRAMES, ids=IDS)
def test_reference_equals_oracle_under_its_flags(oracle_mod, f, flag, rules):
    ok, od, _, _ = _oracle_run(oracle_mod, f, getattr(oracle_mod, flag))
    k, d, _ = _ref(oracle_mod, f, rules)
    assert k.tobytes() == ok.tobytes() and np.array_equal(d, od)


@pytest.mark.parametrize("f", FRAMES, ids=IDS)
def test_planted_keypoints_and_expectations(oracle_mod, f):
    tr = _traces(oracle_mod, f)
    assert len(tr) < f.nfeatures
    for p in f.plants:
        assert (p.level, p.x, p.y) in tr, (p.name, "not a keypoint")
        assert C.realised(f, p, tr[(p.level, p.x, p.y)]) == [], p.name


def _carriers(oracle_mod):
    out = {}
    for f in FRAMES:
        tr = _traces(oracle_mod, f)
        for p in f.plants:
            for it in p.items:
                out.setdefault(it, []).append((f, p, tr[(p.level, p.x, p.y)]))
    return out


def test_census(oracle_mod):
    car = _carriers(oracle_mod)
    # (equal_bit0 and oneapart_bit1 are carried by the constant bands and the tie plants: hand-written values, bit 0
    # for every test between two far samples of a band, bit 1 for the tie's test; realised() checks both)
    # w % 4 = 1 needs a sample 19 columns out: the longest pattern point rounds to 18 at most
    assert float(np.sqrt((R.pattern_points() ** 2).sum(axis=1)).max()) < 18.5
    missing = sorted(set(C.census_items()) - set(car))
    assert missing == sorted(C.UNREACHED), (missing, C.SEARCH)
    # the same patch at the four byte shifts and both row parities: one angle, one descriptor
    grp = [t for (f, p, t) in sum((car[f"sh{i}"] for i in range(4)), []) if f.name == "win320x240"]
    assert len(grp) == 8 and len({(float(t.angle), t.desc.tobytes()) for t in grp}) == 1
    assert grp[0].desc.any() and grp[0].m10 != 0
    # the blur border is live: over the window frames some sample's 7 x 7 support crosses each of the four level-0
    # borders (which samples reach it depends on the texture's angle at each extreme keypoint), and one of level 1
    sides = {0: set(), 1: set()}
    for f in FRAMES:
        if f.name.startswith("win") or f.name == "lvl1":
            tr = _traces(oracle_mod, f)
            for p in f.plants:
                sides[p.level] |= C.border_sides(f, p, tr[(p.level, p.x, p.y)])
    assert sides[0] == {"left", "right", "top", "bottom"} and sides[1], sides
    # both sides of every interior clause were planted, on levels 0 and 1
    for f in FRAMES:
        flags = {p.expect["interior_clauses"] for p in f.plants if "interior_clauses" in p.expect}
        assert flags in (set(), {True, False}), f.name


def _changed(oracle_mod, items, rules):
    """Names of the planted keypoints carrying one of `items` whose angle or descriptor the mutated rule changes."""
    car = _carriers(oracle_mod)
    out = []
    for it in items:
        for (f, p, t) in car.get(it, []):
            m = R.describe(f.levels[p.level], [(p.x, p.y)], p.level, rules)[0]
            if float(m.angle) != float(t.angle) or m.desc.tobytes() != t.desc.tobytes():
                out.append((it, f.name, p.name))
    return out


MUTATIONS = [
    ("uncontracted offsets", R.PINNED._replace(fma=False), ["offset_fma"]),
    ("cvRound half-away", R.PINNED._replace(cvround="away"), ["offset_cvround"]),
    ("correctly rounded trig", R.PINNED._replace(trig="cr"), ["offset_trig"]),
    ("half-up everywhere", R.PINNED._replace(blur="halfup"), ["tie_even_body", "tie_body_w1", "tie_body_w2", "tie_body_w3"]),
    ("half-even everywhere", R.PINNED._replace(blur="halfeven"), ["tie_tail_w2", "tie_tail_w3"]),
    ("parity term dropped", R.PINNED._replace(blur="noparity"), ["tie_odd_body"]),
    ("tail boundary + 1", R.PINNED._replace(tail=1), ["tie_tail_w2", "tie_tail_w3"]),
    ("tail boundary - 1", R.PINNED._replace(tail=-1), ["tie_body_w1", "tie_body_w2", "tie_body_w3"]),
    ("<= for <", R.PINNED._replace(cmp="le"), ["equal_bit0"]),
    ("no saturation", R.PINNED._replace(sat="none"), ["sat_255_256", "sat_256_257"]),
    ("saturation on the left only", R.PINNED._replace(sat="left"), ["sat_255_256", "sat_256_257"]),
    ("replicate border", R.PINNED._replace(border="replicate"),
     ["edge_corner_tl", "edge_corner_tr", "edge_corner_bl", "edge_corner_br"]),
]


@pytest.mark.parametrize("name,rules,items", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutated_rule_changes_its_cases(oracle_mod, name, rules, items):
    """Every item planted for the rule has a keypoint whose output moves (the issue's "saturation on both sides" is
    the reference itself, see describe_ref.saturate_forms: the other one-sided form stands in for it)."""
    hit = {it for (it, _, _) in _changed(oracle_mod, items, rules)}
    assert hit == set(items), (name, sorted(set(items) - hit))


@pytest.mark.parametrize("row", range(16))
def test_mutated_umax_changes_its_row(oracle_mod, row):
    """umax[row] + 1 counts the first pixel outside (the `out` plants of rows +-row leave 90 degrees), umax[row] - 1
    drops the last pixel inside (the `in` plants fall back to 90)."""
    rows = sorted({row, -row})
    for delta, io in ((1, "out"), (-1, "in")):
        items = [f"mask_{io}_v{v}{s}" for v in rows for s in "pn"]
        hit = {it for (it, _, _) in _changed(oracle_mod, items, R.PINNED._replace(umax_row=row, umax_delta=delta))}
        assert hit == set(items), (row, delta, sorted(set(items) - hit))
        other = [f"mask_{io}_v{v}{s}" for v in range(-15, 16) if abs(v) != row for s in "pn"][:8]
        assert _changed(oracle_mod, other, R.PINNED._replace(umax_row=row, umax_delta=delta)) == []
