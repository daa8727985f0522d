"""Planted FAST decisions: the exact arc strength of k_fast_wave / flow_fast on hand-placed 7x7 patterns.

One 320 x 240 frame, flat background, one pattern (or pair) per level-0 cell.  The arc-strength stage holds every
circle value p as the f16 pair (p, -p) taken from the raw byte, so the plants sit where that operand form could go
wrong: p = 0 (the pair (+0, -0)), p = 255 (the largest f16 denormal used), bright-only and dark-only arcs, arcs
that wrap the circle's index 15 -> 0, arc strength exactly at and one above iniThFAST (and at minThFAST in a cell
with nothing at iniThFAST, so the second pass runs), and two adjacent corners of equal strength (the NMS drops both).

Every planted decision is first asserted on the oracle's candidates (a wrong plant fails there), then the GPU's
per-level candidates (orb_debug_candidates) must equal the oracle's on every level, for the per-kernel launches
and for the dataflow launch."""
import numpy as np
import pytest

W, H, BG = 320, 240, 100
INI_TH, MIN_TH = 20, 7
BORDER = 16                     # EDGE_THRESHOLD - 3: candidates are relative to it
W_CELL, H_CELL = 32, 35         # level 0 of 320 x 240: 9 x 6 cells (ORBextractor.cc:781-790)
# the 16 circle offsets (dx, dy) in cv::FAST's order
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def _arc(first, value, rest=BG):
    """Circle values: `value` on the 9-arc that starts at index `first` (wrapping), `rest` elsewhere."""
    ring = [rest] * 16
    for i in range(9):
        ring[(first + i) & 15] = value
    return ring


def _plant(img, x, y, v, ring):
    img[y, x] = v
    for (dx, dy), p in zip(CIRCLE, ring):
        img[y + dy, x + dx] = p


def _strength(img, x, y):
    """max over the 16 9-arcs of the min difference to the centre (bright or dark): corner(th) <=> M > th."""
    v = int(img[y, x])
    p = [int(img[y + dy, x + dx]) for dx, dy in CIRCLE]
    m = 0
    for k in range(16):
        a = [p[(k + i) & 15] for i in range(9)]
        m = max(m, min(a) - v, v - max(a))
    return m


def _cell_origin(i, j):   # first pixel of cell (row i, column j)'s detection domain
    return BORDER + 3 + j * W_CELL, BORDER + 3 + i * H_CELL


def _build():
    """The frame and its plants: (name, x, y, arc strength M, kept as a candidate?)."""
    img = np.full((H, W), BG, np.uint8)
    plants = []

    def one(name, i, j, ox, oy, v, ring, m, kept):
        x0, y0 = _cell_origin(i, j)
        _plant(img, x0 + ox, y0 + oy, v, ring)
        plants.append((name, x0 + ox, y0 + oy, m, kept))

    one("bright only", 0, 0, 16, 17, BG, _arc(2, 160), 60, True)
    one("dark only", 0, 1, 16, 17, BG, _arc(5, 30), 70, True)
    one("bright arc of 255, rest 0", 0, 2, 16, 17, BG, _arc(0, 255, 0), 155, True)
    one("centre 255, dark arc of 0", 0, 3, 16, 17, 255, _arc(3, 0), 255, True)
    one("centre 0, bright arc of 255", 0, 4, 16, 17, 0, _arc(7, 255), 255, True)
    one("centre 255, circle of 0", 0, 5, 16, 17, 255, [0] * 16, 255, True)
    # exactly iniTh (no corner) beside iniTh + 1 (a corner, so the cell stays at iniTh)
    one("M = iniTh", 1, 0, 8, 10, BG, _arc(1, BG + INI_TH), INI_TH, False)
    one("M = iniTh + 1", 1, 0, 24, 25, BG, _arc(1, BG + INI_TH + 1), INI_TH + 1, True)
    one("M = iniTh, dark", 1, 1, 8, 10, BG, _arc(9, BG - INI_TH), INI_TH, False)
    one("M = iniTh + 1, dark", 1, 1, 24, 25, BG, _arc(9, BG - INI_TH - 1), INI_TH + 1, True)
    # the same pair at minTh in a cell with nothing at iniTh: the second pass decides
    one("M = minTh", 1, 2, 8, 10, BG, _arc(4, BG + MIN_TH), MIN_TH, False)
    one("M = minTh + 1", 1, 2, 24, 25, BG, _arc(4, BG + MIN_TH + 1), MIN_TH + 1, True)
    one("M = minTh, dark", 1, 3, 8, 10, BG, _arc(12, BG - MIN_TH), MIN_TH, False)
    one("M = minTh + 1, dark", 1, 3, 24, 25, BG, _arc(12, BG - MIN_TH - 1), MIN_TH + 1, True)
    # 9-arcs across the circle's index 15 -> 0
    one("bright arc 12..4", 2, 0, 16, 17, BG, _arc(12, 160), 60, True)
    one("dark arc 10..2", 2, 1, 16, 17, BG, _arc(10, 30), 70, True)
    one("bright arc 15..7 of 255, rest 0", 2, 2, 16, 17, BG, _arc(15, 255, 0), 155, True)
    # two adjacent corners of equal strength: neither survives the NMS (a strict maximum is required)
    one("equal neighbour, left", 2, 3, 16, 17, BG, _arc(2, 160), 60, False)
    one("equal neighbour, right", 2, 3, 17, 17, BG, _arc(2, 160), 60, False)
    one("equal dark neighbour, upper", 2, 4, 16, 17, BG, _arc(6, 30), 70, False)
    one("equal dark neighbour, lower", 2, 4, 16, 18, BG, _arc(6, 30), 70, False)
    return img, plants


MIN_TH_CELLS = [(1, 2), (1, 3)]   # cells whose plants are all below iniTh


@pytest.fixture(scope="module")
def planted(oracle_mod):
    img, plants = _build()
    o = oracle_mod.OracleExtractor(500, 1.2, 8, INI_TH, MIN_TH)
    assert o.run(img) >= 0
    cands = [o.candidates(l).copy() for l in range(8)]
    return img, plants, cands


def _check_plants(oracle_mod, img, plants, cand0):
    found = {(int(x), int(y)): int(r) for x, y, r in cand0}
    for name, x, y, m, kept in plants:
        assert _strength(img, x, y) == m, (name, "the plant does not have its arc strength")
        key = (x - BORDER, y - BORDER)
        if kept:
            assert found.get(key) == m - 1, (name, "the oracle does not keep the planted corner", found.get(key))
        else:
            assert key not in found, (name, "the oracle keeps a planted non-corner", found[key])
    # the equal neighbours are corners on their own: only the NMS removes them
    by_name = {p[0]: p for p in plants}
    for a, b in [("equal neighbour, left", "equal neighbour, right"),
                 ("equal dark neighbour, upper", "equal dark neighbour, lower")]:
        (_, xa, ya, ma, _), (_, xb, yb, mb, _) = by_name[a], by_name[b]
        assert ma == mb > INI_TH and abs(xa - xb) + abs(ya - yb) == 1
    # the minTh cells: nothing at iniTh in the cell's ROI, the planted corner at minTh
    for i, j in MIN_TH_CELLS:
        x0, y0 = BORDER + j * W_CELL, BORDER + i * H_CELL
        roi = img[y0:y0 + H_CELL + 6, x0:x0 + W_CELL + 6]
        assert len(oracle_mod.fast_roi(roi, INI_TH)) == 0, (i, j)
        assert len(oracle_mod.fast_roi(roi, MIN_TH)) > 0, (i, j)


def test_plants_behave_as_designed_in_the_oracle(oracle_mod, planted):
    """CPU only: every plant has its designed arc strength and the oracle takes the designed decision."""
    img, plants, cands = planted
    _check_plants(oracle_mod, img, plants, cands[0])


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["kernels", "flow"])
def test_planted_candidates_match_oracle(orbgpu_mod, oracle_mod, planted, monkeypatch, launch):
    """The GPU's FAST candidates (x, y, response) of every level equal the oracle's on the planted frame: the
    per-kernel launches (k_fast_wave) and the dataflow launch (flow_fast, the same arc-strength body)."""
    img, plants, cands = planted
    _check_plants(oracle_mod, img, plants, cands[0])
    monkeypatch.setenv("ORBGPU_FLOW", "1" if launch == "flow" else "0")   # read at orb_create
    e = orbgpu_mod.BatchExtractor(500, W, H, 1, ini_th=INI_TH, min_th=MIN_TH)
    try:
        e.upload(img[None])
        e.launch()
        e.sync()
        for l in range(8):
            g = e.debug_candidates(l)
            assert np.array_equal(g, cands[l]), (launch, "FAST candidates differ on level", l, len(g), len(cands[l]))
    finally:
        e.close()


@pytest.mark.gpu
def test_planted_candidates_single_frame_call(orbgpu_mod, oracle_mod, planted):
    """The same through ORBextractor's operator() (the host path's launches)."""
    img, plants, cands = planted
    g = orbgpu_mod.ORBextractor(500, 1.2, 8, INI_TH, MIN_TH)
    g(img)
    for l in range(8):
        assert np.array_equal(g.debug_candidates(l), cands[l]), ("FAST candidates differ on level", l)
