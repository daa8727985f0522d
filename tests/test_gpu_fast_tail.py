"""The prefilter's tail rows in k_fast_wave: rows past a cell's last full row round, one pixel pair per lane.

A cell of two 16-pixel runs per row takes 32 rows per round; the 1-3 rows a 33-35-row cell has beyond that (and
every row of a cell so narrow that all its pixel pairs fit one wave) are compacted from two ballots in place of the
scan.  The image sizes are chosen from the level grid (computed here as ORBextractor.cc:781-806 does) so that
level 0 has cells of exactly 32 (no tail), 33, 34 and 35 rows, a last column narrower than 16 px, of odd width,
and one that runs wholly in tail form; a further multi-level size has 39-row cells (7 leftover rows: too many, the
full round stays) and tail cells on resized levels.  Each case is asserted from the geometry first.

Plants are single dots on a flat background: a dot of value v has arc strength |v - BG| (its whole circle is
background) and its neighbours are no corners.  They sit in the last tail row, at the first and the last valid
pixel of a row (the last pair's high pixel lies past an odd-width domain), in both pixels of one pair with the
stronger one left or right (the NMS keeps the stronger: a lost list entry shows) and across two pairs, and as weak
dots only (a cell that fires the minThFAST pass) with one in a tail row.  Every planted decision is asserted on the
oracle first; then candidates of every level, keypoints and descriptors must equal the oracle's byte for byte, for
the one-frame launch (one cell per wave) and the batch launches (two cells per wave; the dataflow launch too).
Frame 1 of each batch is noise, whose dense survivors fill both ballots in most lanes."""
import math

import numpy as np
import pytest

BG, INI_TH, MIN_TH, NFEAT = 100, 20, 7, 500
BORDER = 16                     # EDGE_THRESHOLD - 3
# (width, height, levels, rows of the level-0 cells of grid row 0)
SIZES = {"rows32": (363, 96, 2, 32), "rows33": (363, 98, 2, 33), "rows34": (363, 100, 2, 34),
         "rows35": (723, 101, 2, 35)}
TEXTURED = (183, 158, 3)


def _level_sizes(w, h, nlevels):
    out, s = [], np.float32(1.0)
    for l in range(nlevels):
        if l:
            s = np.float32(s * np.float32(1.2))
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


def _grid(w, h):
    """Cells of a w x h level: (nCols, wCell, hCell, [(ci, cj, dw, dh, tail rows run as pixel pairs)])."""
    max_bx, max_by = w - BORDER, h - BORDER
    width, height = np.float32(max_bx - BORDER), np.float32(max_by - BORDER)
    ncols, nrows = int(width / np.float32(30)), int(height / np.float32(30))
    wcell, hcell = int(math.ceil(width / ncols)), int(math.ceil(height / nrows))
    cells = []
    for ci in range(nrows):
        for cj in range(ncols):
            ini_y, ini_x = BORDER + ci * hcell, BORDER + cj * wcell
            if ini_y >= max_by - 3 or ini_x >= max_bx - 6:
                continue
            dw = min(ini_x + wcell + 6, max_bx) - ini_x - 6
            dh = min(ini_y + hcell + 6, max_by) - ini_y - 6
            if dw <= 0 or dh <= 0:
                continue
            rpi = 64 // max(1, (dw + 15) // 16)          # rows per round of 16-pixel runs
            left = dh % rpi
            cells.append((ci, cj, dw, dh, left if left * ((dw + 1) // 2) <= 64 else 0))
    return ncols, wcell, hcell, cells


def _build(name):
    """The planted frame of a size: (image, [(x, y, arc strength, kept)], cell of the minTh plants)."""
    w, h, nlevels, rows = SIZES[name]
    ncols, wcell, hcell, cells = _grid(w, h)
    assert hcell == rows and wcell == 31
    img = np.full((h, w), BG, np.uint8)
    plants = []

    def dot(cj, ox, oy, m, kept, ci=0):
        x, y = BORDER + 3 + cj * wcell + ox, BORDER + 3 + ci * hcell + oy
        img[y, x] = BG + m
        plants.append((x, y, m, kept))

    last, dw = rows - 1, 31
    first_tail = 32 if rows > 32 else last
    dot(0, 10, last, 60, True)                                     # the last (tail) row
    dot(1, dw - 1, last, 60, True)                                 # the last valid pixel of a row (pair's low pixel)
    dot(1, 0, first_tail, 50, True)                                # the first pixel of the first tail row
    dot(2, 10, last, 60, True), dot(2, 11, last, 40, False)        # one pair, the left pixel stronger
    dot(3, 12, last, 40, False), dot(3, 13, last, 60, True)        # one pair, the right pixel stronger
    dot(4, 5, 5, 45, True), dot(4, 11, last, 60, True), dot(4, 12, last, 40, False)   # across two pairs, after a full-round entry
    dot(5, 3, 2, 30, True), dot(5, 25, 31, 35, True), dot(5, 0, last, 40, True)       # full rows and tail rows in order
    dot(5, 9, last, 45, True), dot(5, 19, last, 50, True), dot(5, dw - 1, last, 55, True)
    # weak dots only, two cells away from any other plant: the cell fires the minTh pass
    dot(7, 8, 10, 12, True), dot(7, 14, last, 15, True), dot(7, 20, last, 10, False), dot(7, 21, last, 18, True)
    dot(7, 3, first_tail, MIN_TH, False)                           # M = minTh is no corner
    # the last column (narrower than 16 px) and the second grid row (no leftover rows at two runs per row)
    ndw = [c for c in cells if c[0] == 0 and c[1] == ncols - 1][0][2]
    dot(ncols - 1, ndw - 1, last, 60, True), dot(ncols - 1, 0, 3, 50, True)
    dh1 = [c for c in cells if c[0] == 1 and c[1] == ncols - 1][0][3]
    dot(ncols - 1, ndw - 1, dh1 - 1, 60, True, ci=1), dot(ncols - 1, 0, 4, 50, True, ci=1)
    dot(2, 10, dh1 - 1, 60, True, ci=1), dot(2, 11, dh1 - 1, 40, False, ci=1)
    return img, plants, 7


def _noise(w, h, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    img[:, : w // 2] = (img[:, : w // 2] // 8 + 90).astype(np.uint8)   # a low-contrast half: sparse survivors
    return img


def _frames(name):
    if name == "textured":
        from orbgpu.synth import synth_frame
        w, h, nlevels = TEXTURED
        return np.stack([synth_frame(w, h, 3), _noise(w, h, 5), synth_frame(w, h, 4)]), nlevels
    w, h, nlevels, _ = SIZES[name]
    return np.stack([_build(name)[0], _noise(w, h, 11)]), nlevels


def test_level_grids_hold_every_case():
    """CPU only: the sizes' grids have the cells each case needs."""
    tails = {}
    for name, (w, h, nlevels, rows) in SIZES.items():
        ncols, wcell, hcell, cells = _grid(w, h)
        row0 = [c for c in cells if c[0] == 0 and c[1] < ncols - 1]
        assert len(row0) >= 8 and all(c[2] == 31 and c[3] == rows for c in row0), name     # odd width, two runs
        assert all(c[4] == rows - 32 for c in row0), name                                    # 0, 1, 2, 3 tail rows
        tails[name] = rows - 32
        narrow = [c for c in cells if c[1] == ncols - 1]
        assert narrow and all(c[2] < 16 for c in narrow), name
        for lw, lh in _level_sizes(w, h, nlevels):
            assert _grid(lw, lh)[1] <= 36                 # every level at the compact tile pitch
    assert sorted(tails.values()) == [0, 1, 2, 3]
    # the 723-wide size: a last column of odd width 3, its second-row cell (28 rows of 2 pairs) wholly in tail form
    ncols, _, _, cells = _grid(723, 101)
    assert [(c[2], c[3], c[4]) for c in cells if c[1] == ncols - 1] == [(3, 35, 0), (3, 28, 28)]
    # the 363-wide sizes: a last column of odd width 15 (one run per row: 64 rows per round, never a tail)
    assert [(c[2], c[4]) for c in _grid(363, 98)[3] if c[1] == 11 - 1] == [(15, 0), (15, 0)]
    # the multi-level size: tail cells on resized levels, an even width, and 39-row cells whose 7 leftover rows do not fit
    w, h, nlevels = TEXTURED
    seen = set()
    for lw, lh in _level_sizes(w, h, nlevels):
        ncols, wcell, hcell, cells = _grid(lw, lh)
        assert wcell <= 36
        seen |= {(c[2], c[3], c[4]) for c in cells}
    assert {(30, 34, 2), (25, 33, 1), (32, 33, 1), (32, 39, 0), (31, 32, 0)} <= seen


@pytest.fixture(scope="module")
def expected(oracle_mod):
    """Per size: frames, levels and the oracle's candidates / keypoints / descriptors per frame (computed once)."""
    out = {}
    for name in list(SIZES) + ["textured"]:
        frames, nlevels = _frames(name)
        per = []
        for img in frames:
            o = oracle_mod.OracleExtractor(NFEAT, 1.2, nlevels, INI_TH, MIN_TH)
            kps, desc = o(img)
            per.append(([o.candidates(l).copy() for l in range(nlevels)], kps.copy(), desc.copy()))
        out[name] = (frames, nlevels, per)
    return out


def _check_plants(oracle_mod, name, expected):
    img, plants, min_cell = _build(name)
    frames, nlevels, per = expected[name]
    assert np.array_equal(frames[0], img)
    found = {(int(x), int(y)): int(r) for x, y, r in per[0][0][0]}
    for x, y, m, kept in plants:
        key = (x - BORDER, y - BORDER)
        if kept:
            assert found.get(key) == m - 1, (name, x, y, "the oracle does not keep the planted corner", found.get(key))
        else:
            assert key not in found, (name, x, y, "the oracle keeps a planted non-corner")
    assert len(found) == sum(1 for p in plants if p[3]), name
    # the weak cell: nothing at iniTh in its ROI, corners at minTh, one of them in the last row
    w, h, _, rows = SIZES[name]
    x0 = BORDER + min_cell * 31
    roi = np.ascontiguousarray(img[BORDER:BORDER + rows + 6, x0:x0 + 31 + 6])
    assert len(oracle_mod.fast_roi(roi, INI_TH)) == 0 and len(oracle_mod.fast_roi(roi, MIN_TH)) >= 3
    assert any(y == BORDER + 3 + rows - 1 and x0 + 3 <= x < x0 + 3 + 31 and kept for x, y, m, kept in plants)


@pytest.mark.parametrize("name", list(SIZES))
def test_plants_behave_as_designed_in_the_oracle(oracle_mod, expected, name):
    """CPU only: the oracle keeps exactly the dots designed to be kept."""
    _check_plants(oracle_mod, name, expected)


def _compare(e, frame, slot, nlevels, per, what):
    cands, kps, desc = per[frame]
    for l in range(nlevels):
        g = e.debug_candidates(l, slot)
        assert g.tobytes() == cands[l].tobytes(), (what, "FAST candidates differ", "frame", frame, "level", l, len(g),
                                                   len(cands[l]))
    gk, gd = e.results(slot)
    assert len(gk) == len(kps) and gk.tobytes() == kps.tobytes(), (what, "keypoints differ", frame)
    assert gd.tobytes() == desc.tobytes(), (what, "descriptors differ", frame)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES) + ["textured"])
def test_one_frame_launch_matches_oracle(orbgpu_mod, expected, name):
    """One frame per launch: one cell per wave (ipw = 1)."""
    frames, nlevels, per = expected[name]
    h, w = frames[0].shape
    e = orbgpu_mod.BatchExtractor(NFEAT, w, h, 1, nlevels=nlevels, ini_th=INI_TH, min_th=MIN_TH)
    try:
        for f in range(len(frames)):
            e.upload(frames[f][None])
            e.launch()
            e.sync()
            _compare(e, f, 0, nlevels, per, (name, "one frame"))
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["kernels", "flow"])
@pytest.mark.parametrize("name", list(SIZES) + ["textured"])
def test_batch_launch_matches_oracle(orbgpu_mod, expected, monkeypatch, name, launch):
    """A batch of 2-3 frames: two cells per wave (k_fast_wave), and the dataflow launch's flow_fast."""
    frames, nlevels, per = expected[name]
    h, w = frames[0].shape
    monkeypatch.setenv("ORBGPU_FLOW", "1" if launch == "flow" else "0")   # read at orb_create
    e = orbgpu_mod.BatchExtractor(NFEAT, w, h, len(frames), nlevels=nlevels, ini_th=INI_TH, min_th=MIN_TH)
    try:
        e.upload(frames)
        e.launch()
        e.sync()
        for f in range(len(frames)):
            _compare(e, f, f, nlevels, per, (name, launch))
    finally:
        e.close()
