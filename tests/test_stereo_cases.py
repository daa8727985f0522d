"""CPU checks of tests/stereo_cases.py: the restated loop of Frame::ComputeStereoMatches (tests/stereo_ref.py) and the
oracle agree byte for byte on every case, every planted keypoint keeps its window reads inside its level image, and a
census over the reference traces finds every decision of the list (stereo_cases.ITEMS) realised as planted."""
import os

import numpy as np
import pytest

import stereo_cases as sc
import stereo_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VISIBLE = (ref.ACCEPTED, ref.CLAMPED)


def test_constants_agree():
    assert sc.KP_DTYPE.itemsize == 28
    assert (sc.ACCEPTED, sc.CLAMPED, sc.CUT, sc.DIST_HIGH, sc.NO_CANDIDATE, sc.WINDOW_OFF, sc.BEST_AT_L,
            sc.DISPARITY_RANGE) == (ref.ACCEPTED, ref.CLAMPED, ref.CUT, ref.DIST_HIGH, ref.NO_CANDIDATE, ref.WINDOW_OFF,
                                    ref.BEST_AT_L, ref.DISPARITY_RANGE)
    assert ref.c_round(0.5) == 1 and ref.c_round(46.5) == 47 and ref.c_round(-0.5) == -1 and ref.c_round(2.4999) == 2


@pytest.mark.parametrize("name", sc.CASES)
def test_reference_equals_oracle(oracle_mod, name):
    c = sc.case(name)
    u, d, n, _trace = sc.expected(oracle_mod, name)[:4]
    ol, orr = sc.oracle_pair(oracle_mod, c)
    ou, od, on = oracle_mod.stereo_matches(ol, orr, c.kl, c.dl, c.kr, c.dr, c.mb, c.mbf)
    assert n == on, (n, on)
    assert u.tobytes() == ou.tobytes(), np.flatnonzero(u != ou)[:10]
    assert d.tobytes() == od.tobytes()


def test_reference_equals_oracle_on_the_golden_pair(oracle_mod):
    from orbgpu.synth import synth_frame, synth_stereo_right
    g = np.load(os.path.join(GOLDEN, "stereo_640x480.npz"))
    w, h, nf, idx = [int(v) for v in g["cfg"]]
    left = synth_frame(w, h, idx)
    right = synth_stereo_right(left, idx)
    ol, orr = oracle_mod.OracleExtractor(nf), oracle_mod.OracleExtractor(nf)
    kl, dl = ol(left)
    kr, dr = orr(right)
    t = ol.tables()
    u, d, n, trace = ref.compute_stereo_matches([ol.level(l) for l in range(8)], [orr.level(l) for l in range(8)],
                                                t["scale"], t["inv_scale"], kl, dl, kr, dr, float(g["mb"]),
                                                float(g["mbf"]))
    assert n == int(g["n"]) > 20 and u.tobytes() == g["uright"].tobytes() and d.tobytes() == g["depth"].tobytes()
    assert sum(o in VISIBLE for o in trace["outcome"]) == n


def _admitted(c, t, iL):
    """Right keypoints that pass the row band, octave and u gates of left keypoint iL, in iR order, and their
    Hamming distances (a restatement of the gates for the census only)."""
    f32 = np.float32
    r = f32(2.0) * t["scale"][c.kr["octave"]]
    maxr = np.ceil(c.kr["y"] + r)
    minr = np.floor(c.kr["y"] - r)
    row, lv, uL = int(c.kl["y"][iL]), int(c.kl["octave"][iL]), c.kl["x"][iL]
    maxd = f32(f32(c.mbf) / f32(c.mb))
    ok = ((minr <= row) & (row <= maxr) & (np.abs(c.kr["octave"] - lv) <= 1) & (c.kr["x"] >= f32(uL - maxd))
          & (c.kr["x"] <= uL))
    idx = np.flatnonzero(ok)
    dist = np.unpackbits(c.dr[idx] ^ c.dl[iL], axis=1).sum(1) if len(idx) else np.zeros(0, np.int64)
    return idx, dist


@pytest.mark.parametrize("name", sc.CASES)
def test_window_reads_stay_inside_the_levels(oracle_mod, name):
    """Left windows inside their level, every right keypoint that can become a best match at scaled x >= 10 (the
    window search reads 10 columns to its left), row indices and bands inside the image, octaves in range."""
    c = sc.case(name)
    _, _, _, trace, ll, lr, t = sc.expected(oracle_mod, name)
    nlv, H = c.params["nlevels"], ll[0].shape[0]
    assert ll[0].shape == c.left.shape == c.right.shape and [a.shape for a in ll] == [a.shape for a in lr]
    for k in (c.kl, c.kr):
        assert ((k["octave"] >= 0) & (k["octave"] < nlv)).all()
    inv = t["inv_scale"]
    for i in range(len(c.kl)):
        lv = int(c.kl["octave"][i])
        rows, cols = ll[lv].shape
        sx, sy = ref.c_round(c.kl["x"][i] * inv[lv]), ref.c_round(c.kl["y"][i] * inv[lv])
        assert 5 <= sx <= cols - 6 and 5 <= sy <= rows - 6, (name, i, sx, sy, cols, rows)
        assert 0 <= int(c.kl["y"][i]) < H
    if len(c.kr):
        r = np.float32(2.0) * t["scale"][c.kr["octave"]]
        assert (np.floor(c.kr["y"] - r) >= 0).all() and (np.ceil(c.kr["y"] + r) < H).all()   # vRowIndices[yi] exists
        # right keypoints near a left keypoint's gates (two rows, two octaves, one pixel wider than the gates, so the
        # decoys are among them): a search that took one would read 10 columns to the left of its scaled x
        maxd = np.float32(np.float32(c.mbf) / np.float32(c.mb))
        lo_r, hi_r = np.floor(c.kr["y"] - r) - 2, np.ceil(c.kr["y"] + r) + 2
        for i in range(len(c.kl)):
            lv, row, uL = int(c.kl["octave"][i]), int(c.kl["y"][i]), c.kl["x"][i]
            near = ((lo_r <= row) & (row <= hi_r) & (np.abs(c.kr["octave"] - lv) <= 2)
                    & (c.kr["x"] >= uL - maxd - 1) & (c.kr["x"] <= uL + 1))
            sx = np.floor(c.kr["x"][near] * inv[lv] + np.float32(0.5))
            assert (sx >= 10).all(), (name, i, np.flatnonzero(near)[sx < 10])
    assert len(trace["outcome"]) == len(c.kl)


def test_case_shapes():
    c = sc.case("levels_odd_strided")
    h, w = c.left.shape
    assert w % 2 == 1 and h % 2 == 1
    assert c.left.strides == (w + 29, 1) and c.right.strides == (w + 61, 1)
    p = sc.case("levels_pyr2").params
    assert p["scaleFactor"] == 2.0 and p["nlevels"] == 3
    p = sc.case("levels_pyr15").params
    assert int(np.ceil(2.0 * p["scaleFactor"] ** (p["nlevels"] - 1))) + 1 == 8   # the bucket lookup's reach: not 9
    assert len(sc.case("nr_zero").kr) == 0 and len(sc.case("nr_zero").kl) > 0
    assert len(sc.case("nl_one").kl) == 1
    assert len(sc.case("search").kl) % 4 != 0 and len(sc.case("many").kl) > 256
    b = sc.case("big_nr")
    assert 65536 < len(b.kr) <= 65700 and b.dr.nbytes < 2.2e6
    for c in (sc.case(n) for n in sc.CASES):
        assert max(c.left.shape) <= 416, c.name


def test_census(oracle_mod):
    """Every item of the list is planted by some case, and the reference trace shows it as planted."""
    seen = {}
    for name in sc.CASES:
        c = sc.case(name)
        _, _, nmatched, tr, _, _, t = sc.expected(oracle_mod, name)
        assert nmatched == sum(o in VISIBLE for o in tr["outcome"])
        if name in sc.MEDIANS:
            assert tr["median"] == sc.MEDIANS[name], (name, tr["median"])
        for p in c.plants:
            ctx = (name, p)
            i = p.iL
            if p.best_idx is not None:
                assert tr["best_idx"][i] == p.best_idx, (ctx, tr["best_idx"][i])
            if p.best_dist is not None:
                assert tr["best_dist"][i] == p.best_dist, (ctx, tr["best_dist"][i])
            if p.outcome is not None:
                assert tr["outcome"][i] == p.outcome, (ctx, tr["outcome"][i], tr["vdists"][i])
            if p.visible:
                assert tr["outcome"][i] in VISIBLE, (ctx, tr["outcome"][i], tr["vdists"][i], tr["median"])
            if p.bestinc is not None:
                assert tr["bestinc"][i] == p.bestinc, (ctx, tr["bestinc"][i], tr["vdists"][i])
            if p.sad is not None:
                # the planted window distance is the minimum over the 11 offsets and what the cut saw
                assert np.nanmin(tr["vdists"][i]) == p.sad, (ctx, tr["vdists"][i])
                assert tr["outcome"][i] not in VISIBLE + (ref.CUT,) or tr["sad"][i] == p.sad, ctx
            if p.best_idx is not None and p.best_idx >= 0:
                # every other right keypoint at Hamming distance 0 or at the best distance (decoys, tie partners) lies
                # at least 12 scaled pixels from the chosen one
                d_all = np.unpackbits(c.dr ^ c.dl[i], axis=1).sum(1)
                rivals = np.flatnonzero((d_all == 0) | (d_all == tr["best_dist"][i]))
                rivals = rivals[(rivals != p.best_idx) & (c.kr["x"][rivals] != c.kr["x"][p.best_idx])]
                gap = np.abs(c.kr["x"][rivals] - c.kr["x"][p.best_idx]) * t["inv_scale"][c.kl["octave"][i]]
                assert (gap >= 12).all(), (ctx, rivals, gap)
            seen.setdefault(p.item, []).append((name, p, tr))
        # per-item structure that the trace alone does not show
        for p in c.plants:
            i = p.iL
            idx, dist = _admitted(c, t, i)
            if p.item.startswith("tie_"):
                tied = idx[dist == p.best_dist]
                assert len(tied) >= 2 and tied[0] == p.best_idx and dist.min() == p.best_dist, (name, p, tied)
                if p.item == "tie_lower_ir_later_row":
                    assert np.floor(c.kr["y"][tied[0]]) > np.floor(c.kr["y"][tied[1]])
                if p.item == "tie_beyond_64":
                    assert len(idx) > 64 and np.flatnonzero(idx == p.best_idx)[0] >= 64
                    assert len(set(np.floor(c.kr["y"][idx]).tolist())) == 1      # one bucket row: position = rank
            if "decoy" in p.item or p.item.endswith(("past_maxr", "before_minr")):
                d_all = np.unpackbits(c.dr ^ c.dl[i], axis=1).sum(1)
                decoys = np.flatnonzero(d_all == 0)
                assert len(decoys) >= 1 and not np.isin(decoys, idx).any(), (name, p, decoys)
            if p.item.endswith(("at_maxr", "at_minr")):
                k = p.best_idx
                r = np.float32(2.0) * t["scale"][c.kr["octave"][k]]
                edge = np.ceil(c.kr["y"][k] + r) if p.item.endswith("at_maxr") else np.floor(c.kr["y"][k] - r)
                assert edge == int(c.kl["y"][i]) and c.kr["y"][k] != np.floor(c.kr["y"][k])
                assert c.kr["octave"][k] == (0 if "_o0_" in p.item else c.params["nlevels"] - 1)
            if p.item.endswith(("past_maxr", "before_minr")):
                k = np.flatnonzero(np.unpackbits(c.dr ^ c.dl[i], axis=1).sum(1) == 0)[0]
                r = np.float32(2.0) * t["scale"][c.kr["octave"][k]]
                edge = np.ceil(c.kr["y"][k] + r) + 1 if p.item.endswith("past_maxr") else np.floor(c.kr["y"][k] - r) - 1
                assert edge == int(c.kl["y"][i])
                assert c.kr["octave"][k] == (0 if "_o0_" in p.item else c.params["nlevels"] - 1)
            if p.item in ("u_at_maxu", "u_at_minu"):
                maxd = np.float32(np.float32(c.mbf) / np.float32(c.mb))
                want = c.kl["x"][i] if p.item == "u_at_maxu" else np.float32(c.kl["x"][i] - maxd)
                assert c.kr["x"][p.best_idx] == want
            if p.item.startswith("partner_level"):
                assert c.kr["octave"][p.best_idx] - c.kl["octave"][i] == (-1 if "minus" in p.item else 1)
            if p.item.startswith("octave_decoy"):
                k = np.flatnonzero(np.unpackbits(c.dr ^ c.dl[i], axis=1).sum(1) == 0)
                assert (c.kr["octave"][k] - c.kl["octave"][i] == (-2 if "minus" in p.item else 2)).any()
            if p.item in ("clamp_row_0", "clamp_row_last"):
                reach = int(np.ceil(2.0 * t["scale"][-1])) + 1
                row = int(c.kl["y"][i])
                assert row - reach < 0 if p.item == "clamp_row_0" else row + reach > c.left.shape[0] - 1
            if p.item == "fractional_vl":
                assert int(c.kl["y"][i]) + 1 == ref.c_round(c.kl["y"][i]) and len(idx) == 1
                assert not (np.floor(c.kr["y"][idx] - 2) <= int(c.kl["y"][i]) + 1 <= np.ceil(c.kr["y"][idx] + 2))
            if p.item == "no_candidate":
                assert tr["ncand"][i] == 0
            if p.item == "dist_100":
                assert 100 in dist.tolist() and dist.min() == 100
            if p.item == "equal_minimum_lower_offset":
                v = tr["vdists"][i]
                assert v[2] == v[5] == v[8] == v.min()
            if p.item in ("endu_cols", "endu_cols_minus1"):
                x = ref.c_round(c.kr["x"][p.best_idx])
                assert x + 11 == c.left.shape[1] - (p.item == "endu_cols_minus1")
            if p.item == "zero_disparity":
                assert c.kr["x"][p.best_idx] == c.kl["x"][i] and tr["vdists"][i][4] == tr["vdists"][i][6]
            if p.item == "disparity_at_maxd":
                maxd = np.float32(np.float32(c.mbf) / np.float32(c.mb))
                v = tr["vdists"][i]
                assert c.kl["x"][i] - c.kr["x"][p.best_idx] == maxd and v[4] == v[6] and v[5] == 0
            if p.item.endswith("_kept_below_th") or p.item.endswith("_cut_at_th"):
                # one distance on each side of thDist of the right median: the neighbouring medians move one of them
                assert (np.float32(p.sad) < np.float32(tr["th_dist"])) == p.item.endswith("_kept_below_th")
                assert abs(p.sad - tr["th_dist"]) <= 1
            if p.item == "negative_disparity":
                assert 0 < c.kl["x"][i] - c.kr["x"][p.best_idx] < 0.5 < c.kr["x"][p.best_idx] % 1
            if p.item.startswith("octave_gt0") or p.item == "half_rounding":
                assert c.kl["octave"][i] > 0
            if p.item == "half_rounding":
                lv = c.kl["octave"][i]
                assert (c.kl["x"][i] * t["inv_scale"][lv]) % 1 == 0.5 and (c.kr["x"][p.best_idx] * t["inv_scale"][lv]) % 1 == 0.5
            if p.item == "sad_above_32768":
                sads = tr["sad"][tr["sad"] >= 0]
                assert len(sads) >= 3 and (sads > 32768).all()
            if p.item == "accepted_index_above_256":
                assert i > 256
            if p.item == "right_index_above_65535":
                assert p.best_idx >= 65536 and c.kr["x"][p.best_idx & 0xFFFF] != c.kr["x"][p.best_idx]
                assert len(idx) == 1                      # the filler is never admitted
            if p.item.startswith("cut_"):
                assert tr["outcome"][i] in (ref.ACCEPTED, ref.CUT)
                assert (tr["outcome"][i] == ref.CUT) == (np.float32(p.sad) >= np.float32(tr["th_dist"]))
    missing = [it for it in sc.ITEMS if it not in seen]
    assert not missing, missing
    assert set(seen) == set(sc.ITEMS)
    for item in ("octave_gt0_default", "octave_gt0_pyr2", "octave_gt0_pyr15"):
        assert sum(tr["outcome"][p.iL] == ref.ACCEPTED for _, p, tr in seen[item]) >= 5, item
    # the float comparison of the cut: one below 2.1 * median is kept, one above is cut
    for v in (21, 42, 210):
        assert seen[f"cut_{v}_{v - 1}"][0][2]["outcome"][seen[f"cut_{v}_{v - 1}"][0][1].iL] == ref.ACCEPTED
        assert seen[f"cut_{v}_{v + 1}"][0][2]["outcome"][seen[f"cut_{v}_{v + 1}"][0][1].iL] == ref.CUT
    # first / last element of the median's low-byte bucket: the rank of the median among its equals
    for item, want in (("median_first_of_bucket", 0), ("median_last_of_bucket", -1)):
        name, _, tr = seen[item][0]
        sads = np.sort(tr["sad"][tr["sad"] >= 0])
        equal = np.flatnonzero(sads == tr["median"])
        assert len(equal) >= 2 and len(sads) // 2 == equal[want], (item, sads)
    name, _, tr = seen["median_ties"][0]
    assert (tr["sad"] == tr["median"]).sum() >= 5
    assert all(o == ref.CUT for o in seen["median_zero"][0][2]["outcome"])
    assert all(o == ref.ACCEPTED for o in seen["median_all_equal"][0][2]["outcome"])
    assert len(sc.case("median_odd").kl) % 2 == 1 and len(sc.case("median_even").kl) % 2 == 0
