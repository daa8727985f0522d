"""CPU checks of tests/bird_cases.py: the plain reference (tests/bird_ref.py) realises every plant; its integer stages
equal the oracle (candidate positions, FAST scores, level images, blurred images, one-level descriptors, keep / cull
sets); its float stages agree with the oracle within the stated bounds (Harris: 2^-20 (ixx + iyy)^2 scale^4; angles:
0.3 degrees, exact at the special points; cornerSubPix: measured, see bird_cases.SUBPIX_*); every trace item of
cornerSubPix shows the exit or regime it is named for.  test_census lists every item as realised; none is skipped."""
import numpy as np
import pytest

import bird_cases as bc
import bird_ref as ref

REALISED = {}


def _mark(case, items=None):
    for it in items if items is not None else {p.item for p in case.plants}:
        REALISED.setdefault(it, set()).add(case.name)


def _nper(case):
    return ref.features_per_level(case.nfeat, case.nlevels)


def _oracle(oracle_mod, case):
    return oracle_mod.OracleCvORB(case.nfeat, 1.2, case.nlevels)


@pytest.mark.parametrize("name", [c.name for c in bc.by_kind("detect")])
def test_detect_case(oracle_mod, name):
    case = bc.cases()[name]
    mask = ref.footprint_mask(case.mask) if name == "footprint" else case.mask
    sel, cands, lv = ref.detect_set(case.img, mask, _nper(case), case.nlevels)
    o = _oracle(oracle_mod, case)
    kps = o.detect(case.img, mask)
    ocands = [o.candidates(l) for l in range(case.nlevels)]
    scales = [s for _, _, s in ref.level_sizes(case.img.shape[1], case.img.shape[0], case.nlevels)]
    # integer stages: level images, candidate positions and FAST scores, the keep set
    for l in range(case.nlevels):
        assert np.array_equal(lv[l], o.level(l)), l
        assert [(int(c["x"]), int(c["y"]), int(c["class_id"])) for c in ocands[l]] == cands[l], l
        for c in ocands[l]:      # float stage: the Harris response from the exact sums
            s = ref.harris_sums(lv[l], int(c["x"]), int(c["y"]))
            assert abs(ref.harris_response(s) - float(c["response"])) <= ref.harris_bound(s), (l, c, s)
    f = np.float32
    want = {(l, float(f(x) * f(scales[l])), float(f(y) * f(scales[l]))) for l, x, y in sel}
    assert {(int(k["octave"]), float(k["x"]), float(k["y"])) for k in kps} == want
    # the plants in the reference: raw scores and candidates, counts, moments, Harris sums
    sc = [ref.fast_scores(x) for x in lv]
    for p in case.plants:
        if p.what == "cand":
            l, x, y = p.where
            assert (((x, y, int(sc[l][y, x])) in cands[l]), int(sc[l][y, x])) == p.expect, p
            if p.item == "mask_254_drops_level1":      # the resized mask before the threshold
                w1, h1, _ = ref.level_sizes(bc.W8, bc.H8, 2)[1]
                m1 = ref.resize_linear(case.mask, w1, h1)
                assert m1[y, x] == (255 if p.expect[0] else 254) and case.mask.min() > 0 and (case.mask < 255).sum() == 2, p
        elif p.what == "count":
            assert sum(w in sel for w in p.where) == p.expect, p
        elif p.what == "harris":
            l, x, y = p.where
            s = ref.harris_sums(lv[l], x, y)
            assert (s[0] > 2 ** 24 and ref.harris_response(s) > 0) if p.expect == "above_2p24" else ref.harris_response(s) < 0, (p, s)
        elif p.what == "angle":
            l, x, y = p.where
            m10, m01 = ref.moments(lv[l], x, y)
            if p.expect[0] == "near":
                assert (m10, m01) == p.expect[1:], (p, m10, m01)
            else:
                assert abs(ref.angle_deg(m10, m01) % 360.0 - float(p.expect[1]) % 360.0) < 0.3, (p, m10, m01)
                assert oracle_mod.fast_atan2(float(m01), float(m10)) == p.expect[1], p      # the stated float is the oracle's
                if p.item == "angle_symmetric_zero":
                    assert m10 == 0 and m01 == 0
                elif p.item == "angle_axes":
                    assert (m10 == 0) != (m01 == 0)
                elif p.item == "angle_diagonals":
                    assert abs(m10) == abs(m01) != 0
    if name.startswith("retain_ties"):
        assert len(kps) == 8 > case.nfeat
    if name == "retain_margin":      # the exact gap exceeds the float bound of either group
        rs = {k: [ref.harris_sums(lv[0], x, y) for x, y in g] for k, g in (("s", bc.MARGIN_STRONG), ("w", bc.MARGIN_WEAK))}
        gap = min(map(ref.harris_response, rs["s"])) - max(map(ref.harris_response, rs["w"]))
        assert gap > max(ref.harris_bound(s) for s in rs["s"] + rs["w"]), gap
    # the plants in the oracle's output
    assert not bc.detect_failures(case, ocands, kps)
    if name == "footprint":
        ke, _ = o.extract(case.img, case.mask)
        assert not bc.extract_failures(case, ke)
        assert len(ke) == sum(p.expect for p in case.plants)
    # angles of every keypoint against float64 atan2 (OpenCV documents 0.3 degrees for fastAtan2)
    dev = 0.0
    for k in kps:
        l = int(k["octave"])
        m10, m01 = ref.moments(lv[l], int(round(float(k["x"]) / scales[l])), int(round(float(k["y"]) / scales[l])))
        d = abs(float(k["angle"]) - ref.angle_deg(m10, m01))
        dev = max(dev, min(d, 360.0 - d))
    assert dev < 0.3
    print("largest fastAtan2 deviation in %s: %.4f degrees" % (name, dev))
    _mark(case)


def _oracle_follows(oracle_mod, img, s, reach):
    """The oracle's path is the float64 trace's, as far as its output shows: with maxCount = n it returns the position
    after n iterations while that is within 5 px of the start (here: within 1e-3 of the trace) and the start itself
    beyond.  From the last visible position (as float32) both are started again, until the chain of visible
    positions is more than `reach` px from the first start."""
    start = np.asarray(s, np.float32)
    for _ in range(6):
        _, tr, _ = ref.corner_subpix(img, start)
        last = 0
        for n in range(1, len(tr)):
            got = oracle_mod.corner_subpix(img, start[None], max_iter=n)[0]
            if tr[n]["off"] < 4.99:
                assert max(abs(got[0] - tr[n]["pos"][0]), abs(got[1] - tr[n]["pos"][1])) < 1e-3, (start, n, got, tr[n])
                last = n
            elif tr[n]["off"] > 5.01:
                assert got.tobytes() == start.tobytes(), (start, n, got)
        assert last > 0
        nxt = np.array(tr[last]["pos"], np.float32)
        if max(abs(float(nxt[0]) - float(s[0])), abs(float(nxt[1]) - float(s[1]))) > reach:
            return
        start = nxt
    raise AssertionError("the oracle's visible path does not reach %g px from %r" % (reach, s))


def _subpix_check(oracle_mod, case, only=None):
    out = oracle_mod.corner_subpix(case.img, case.pts)
    to_ref = to_analytic = 0.0
    for p in case.plants:
        if only and p.item != only:
            continue
        s, e = case.pts[p.where], p.expect
        (rx, ry), tr, reset = ref.corner_subpix(case.img, s)
        if "exit" in e:
            assert tr[-1]["exit"] == e["exit"], (p, tr[-1])
        if "iters" in e:
            assert len(tr) == e["iters"], (p, len(tr))
        if "reset" in e:
            assert reset == e["reset"], p
        if e.get("outside"):
            assert ry < 0, p
        if "inside_first" in e:
            assert tr[0]["inside"] == e["inside_first"], p
        if e.get("uncached"):      # inside, but a 32 x 32 neighbourhood around the start would cross the image edge
            assert 8 <= s[0] < 15 and tr[0]["inside"], p
        if e.get("integer_start"):
            assert tr[0]["integer_x"] and not tr[1]["integer_x"], p
        if e.get("leaves_cache"):   # iterations, not the last, inside the image but outside the start's 32 x 32 pixels
            assert all(t["inside"] for t in tr), p
            far = [i for i, t in enumerate(tr[:-1]) if not bc.in_start_neighbourhood(s, t["ipx"], t["ipy"])]
            assert len(far) >= 3 and max(t["off"] for t in tr) > 9, (p, far)
            _oracle_follows(oracle_mod, case.img, s, 9.0)
        if p.item == "subpix_reset_over_5px":
            assert tr[-1]["exit"] == ref.EPS and max(t["off"] for t in tr) < 9, p
            assert all(bc.in_start_neighbourhood(s, t["ipx"], t["ipy"]) for t in tr), p
            _oracle_follows(oracle_mod, case.img, s, 5.0)
        if p.item == "subpix_40_iterations":      # the oracle too: one iteration fewer or more gives another result
            for n in (39, 41):
                assert oracle_mod.corner_subpix(case.img, s[None], max_iter=n).tobytes() != out[p.where].tobytes(), (p, n)
        if "analytic" in e:
            to_ref = max(to_ref, abs(out[p.where][0] - rx), abs(out[p.where][1] - ry))
            to_analytic = max(to_analytic, abs(out[p.where][0] - e["analytic"][0]), abs(out[p.where][1] - e["analytic"][1]))
    bad = [b for b in bc.subpix_failures(case, out) if not only or b[0] == only]
    assert not bad, bad
    return to_ref, to_analytic


@pytest.mark.parametrize("name", [c.name for c in bc.by_kind("subpix")])
def test_subpix_case(oracle_mod, name):
    case = bc.cases()[name]
    _subpix_check(oracle_mod, case)
    _mark(case)


def test_subpix_ideal_corner_bounds(oracle_mod):
    """The measured distances that bird_cases.SUBPIX_* record (run with -s to see them)."""
    to_ref, to_analytic = _subpix_check(oracle_mod, bc.cases()["subpix"], None)
    print("subpix_ideal: oracle to bird_ref %.3g px, oracle to the analytic corner %.3g px" % (to_ref, to_analytic))
    assert to_ref <= bc.SUBPIX_ORACLE_TO_REF and to_analytic <= bc.SUBPIX_ORACLE_TO_ANALYTIC


@pytest.mark.parametrize("name", [c.name for c in bc.by_kind("compute")])
def test_compute_case(oracle_mod, name):
    case = bc.cases()[name]
    o = _oracle(oracle_mod, case)
    ko, do = o.compute(case.img, case.kps)
    assert not bc.compute_failures(case, ko, do)
    if case.nlevels == 1:       # the blurred image is the oracle's
        assert np.array_equal(ref.blur(case.img), oracle_mod.blur(case.img))
    for p in case.plants:
        e = p.expect
        if p.what == "blur":     # an exact half with the stated quotient, rounded by its column's rule
            x, y, level = p.where if len(p.where) == 3 else p.where + (0,)
            lv = ref.pyramid(case.img, level + 1)[level]
            s = int(ref.blur_sums(lv)[y, x])
            assert s == e[0] * 65536 + 32768 and int(ref.blur(lv)[y, x]) == e[1], (p, s)
            assert e[1] == (e[0] + 1 if x >= (lv.shape[1] & ~3) else e[0] + (e[0] & 1)), p
            assert np.array_equal(ref.blur(lv), oracle_mod.blur(lv))
        elif p.what == "desc" and "other_rule" in e:     # the other rounding rule on that column would flip the bit
            k = case.kps[p.where]
            other, _ = ref.descriptor(bc.blurred(case.name, int(k["octave"]), e["other_rule"]), *bc.level_xy(case, k),
                                      float(k["angle"]))
            assert (other[e["pair"] // 8] >> (e["pair"] % 8)) & 1 == 1 - e["bit"], p
        elif p.what == "desc" and "sides" in e:     # samples beyond the level on one / two sides
            k = case.kps[p.where]
            w, h, sc = ref.level_sizes(bc.W8, bc.H8, 8)[int(k["octave"])]
            cx, cy = int(np.rint(k["x"] / np.float32(sc))), int(np.rint(k["y"] / np.float32(sc)))
            out_x, out_y = cx - 13 < 0 or cx + 13 >= w, cy - 13 < 0 or cy + 13 >= h
            n_out = bc._samples_outside(float(k["x"]), float(k["y"]), float(k["angle"]), int(k["octave"]))
            assert out_x + out_y == e["sides"] and n_out > 0, (p, cx, cy, w, h, n_out)
    if name == "blur":
        assert sorted(p.expect[0] % 2 for p in case.plants if p.what == "blur") == [0, 0, 1]
    if name == "blur_tail":     # a tail column, reached by the keypoint's second sample of the planted pair
        (x, y, level), k = case.plants[0].where, case.kps[0]
        ox, oy = ref.sample_offsets(90.0)
        cx, cy = bc.level_xy(case, k)
        assert x >= (ref.level_sizes(bc.W8, bc.H8, level + 1)[level][0] & ~3)
        assert (cx + ox[2 * bc.TAIL_PAIR + 1], cy + oy[2 * bc.TAIL_PAIR + 1]) == (x, y)
    _mark(case)


def test_census(oracle_mod, capsys):
    """Every item of bird_cases.ITEMS is planted, and realised by the tests above (run here again if this test runs
    alone)."""
    for c in bc.cases().values():
        if not all(c.name in REALISED.get(p.item, ()) for p in c.plants):
            {"detect": test_detect_case, "subpix": test_subpix_case, "compute": test_compute_case}[c.kind](oracle_mod, c.name)
    planted = {p.item for c in bc.cases().values() for p in c.plants}
    assert planted == set(bc.ITEMS), (planted ^ set(bc.ITEMS))
    missing = [it for it in bc.ITEMS if it not in REALISED]
    with capsys.disabled():
        print()
        for it in bc.ITEMS:
            print("  %-36s %s" % (it, "realised in " + ", ".join(sorted(REALISED[it])) if it in REALISED else "MISSING"))
        print("  %d of %d items realised, 0 skipped" % (len(bc.ITEMS) - len(missing), len(bc.ITEMS)))
    assert not missing, missing
    for c in bc.cases().values():
        assert c.img.shape[0] <= 240 and c.img.shape[1] <= 320
