"""The ROI staging of k_fast_wave / flow_fast by format loads (csrc/extract_kernels.hip: fast_roi_issue,
fast_roi_store): FAST candidates of every level, keypoints and descriptors equal the oracle's byte for byte.

An aligned level's ROI row is loaded as groups of four pixels from ROI column -1 on (group ww = columns 4 ww - 1 ..
4 ww + 2, nw = ceil((rw + 1) / 4) groups a row, rpr = 64 // nw rows a round, 8 rounds prefetched, later rows loaded in
the store); each group arrives widened to 16 bits and is one 8-byte store at tile elements 4 ww .. 4 ww + 3.  The
forms of that store, restated here from the cells of tests/fast_stage_cases.py's geometry model and asserted on the
CPU (test_sizes_cover_every_store_form):

    the load address (iniX - 1) at each of the four byte alignments (iniX & 3 = 0, 1, 2, 3)
    a row's last group holding 1, 2, 3 and 4 pixels of the row (columns -1 .. rw - 1), at both tile pitches
    the tile pitches 48 and 80
    a tall ROI (rh > 8 rpr) at both pitches: the seam between the prefetched rows and the rows loaded in the store
    a frame whose stride is no multiple of 4: BatchExtractor stores it byte by byte

The sizes are fast_stage_cases' five, 100 x 91 (pitch 48: ROI 40 wide, whose last group holds only column rw - 1,
and 34 wide; both 59 rows tall, rows 40.. / 56.. loaded in the store) and 180 x 110 (pitch 80, 4 x 2 cells of 37 x 39,
ROI 43 x 45 in grid row 0 at all four alignments: rows 40.. loaded in the store, in a carve small enough for the
dataflow launch).

Frames of a size (level 0 planted, flat background BG):

    edge0/1  the first and last ROI column and the first and last ROI row of every cell alternate 0 and 255 (edge1:
             255 and 0): a wrong pair order, a dropped last element or a missing zero changes a corner's score
    arcs     per cell four centres BG - 11 under a 9-arc of BG + 10 (strength iniTh + 1) at domain (0, 8),
             (dw - 1, 18), (6, 0) and (14, dh - 1): each arc holds the three circle pixels of the ROI's outermost column
             or row, and losing any pixel of a 9-arc of iniTh + 1 loses the corner
    noise    two noise frames

Each size runs as one frame per launch, as batches of B = 3 of its frames (two cells per wave, a wave's pair of cells
straddling two frames), through ORBextractor's operator(), and through the dataflow launch, whose FAST stage takes the
same loads at its own cache policy.  That launch takes at most two frames, so it runs batches of B = 2, and only
geometries whose FAST carve fits a CU 16 times (build_flow; the 59-row cells of the other sizes do not, and silently
run the per-kernel launches): 364 x 101 (pitch 48, every alignment, late rows at level 1) and 180 x 110 (pitch 80,
every alignment, late rows).  Its task stamps are read to show that it, not the per-kernel launches, ran."""
import pytest

import fast_stage_cases as fc
from test_fast_arc_planted import _arc, _plant, _strength
from gpu_tools import flow_task_ends
from test_gpu_fast_tail import BORDER, _noise

BG = fc.BG
SIZES = dict(fc.SIZES, w100=(100, 91, 1), w180h110=(180, 110, 1))
NAMES = list(SIZES)
# the sizes whose per-wave LDS carve lets 16 waves share a CU, which the dataflow launch needs (_flow_fits)
FLOW_NAMES = ["w364", "w180h110"]
# (domain x, domain y, first index of the 9-arc in CIRCLE): the arcs through column -3, column +3, row -3, row +3
ARCS = [(lambda c: (0, 8), 8), (lambda c: (c.dw - 1, 18), 0), (lambda c: (6, 0), 4), (lambda c: (14, c.dh - 1), 12)]


def _store_form(c):
    """(groups a row, rows a round, pixels of the row in its last group, rows loaded in the store?)"""
    nw = (c.rw + 1 + 3) // 4
    rpr = 64 // nw
    return nw, rpr, c.rw + 1 - 4 * (nw - 1), c.rh > 8 * rpr


def _edge_frame(geo, phase):
    import numpy as np
    img = np.full((geo.h, geo.w), BG, np.uint8)
    for c in geo.levels[0].cells:
        for y in range(c.ini_y, c.ini_y + c.rh):
            img[y, c.ini_x] = img[y, c.ini_x + c.rw - 1] = 255 * ((y + phase) & 1)
        for x in range(c.ini_x, c.ini_x + c.rw):
            img[c.ini_y, x] = img[c.ini_y + c.rh - 1, x] = 255 * ((x + phase) & 1)
    return img


def _arc_frame(geo):
    import numpy as np
    img = np.full((geo.h, geo.w), BG, np.uint8)
    centres = []
    for c in geo.levels[0].cells:
        x0, y0 = c.origin()
        for at, first in ARCS:
            ox, oy = at(c)
            if ox < c.dw and oy < c.dh:
                _plant(img, x0 + ox, y0 + oy, BG - 11, _arc(first, BG + 10))
                centres.append((x0 + ox, y0 + oy))
    return img, centres


_CASES = {}


def _case(oracle_mod, name):
    """(geometry, frames, arc centres, per frame the oracle's (candidates per level, keypoints, descriptors)): computed
    once per size and shared by every test."""
    import numpy as np
    if name not in _CASES:
        w, h, nlevels = SIZES[name]
        geo = fc.Geometry(w, h, nlevels)
        arcs, centres = _arc_frame(geo)
        frames = np.stack([_edge_frame(geo, 0), _edge_frame(geo, 1), arcs, _noise(w, h, 23), _noise(w, h, 24)])
        per = []
        for img in frames:
            o = oracle_mod.OracleExtractor(fc.NFEAT, 1.2, geo.nlevels, fc.INI_TH, fc.MIN_TH)
            kps, desc = o(img)
            per.append(([o.candidates(l).copy() for l in range(geo.nlevels)], kps.copy(), desc.copy()))
        _CASES[name] = (geo, frames, centres, per)
    return _CASES[name]


ARC_FRAME = 2


def _flow_fits(geo):
    """build_flow / fast_wave_layout restated: 16 waves' carves (tile rows of the tallest cell + 6, the survivor list of
    the largest cell) within 160 KiB - 64."""
    rows = max(L.hcell for L in geo.levels) + 6
    lst = max(L.hcell * L.wcell for L in geo.levels)
    wave = ((rows * geo.pitch * 2 + 32 + 15) & ~15) + ((lst * 2 + 15) & ~15)
    return 16 * wave <= 160 * 1024 - 64


def test_dataflow_sizes_cover_the_store_forms():
    """CPU only: the sizes the dataflow launch takes are FLOW_NAMES, and they reach both pitches, every alignment of
    the load address and a tall ROI at each pitch."""
    assert [n for n in NAMES if _flow_fits(fc.Geometry(*SIZES[n]))] == FLOW_NAMES
    align, tall = set(), set()
    for name in FLOW_NAMES:
        geo = fc.Geometry(*SIZES[name])
        assert geo.level0_aligned(geo.w)
        for c in geo.cells():
            align.add((geo.pitch, c.ini_x & 3))
            if _store_form(c)[3]:
                tall.add(geo.pitch)
    assert align == {(p, a) for p in (fc.PITCH_COMPACT, fc.PITCH_WIDE) for a in range(4)}
    assert tall == {fc.PITCH_COMPACT, fc.PITCH_WIDE}


def test_sizes_cover_every_store_form():
    """CPU only: the sizes reach every form of the store named in the module docstring."""
    align, last, tall, pitches, byte_path = set(), set(), set(), set(), set()
    for name, (w, h, nlevels) in SIZES.items():
        geo = fc.Geometry(w, h, nlevels)
        pitches.add(geo.pitch)
        if not geo.level0_aligned(w):
            byte_path.add(name)
        for c in geo.cells():
            if c.level == 0 and not geo.level0_aligned(w):
                continue   # (aligned through operator(); counted from the aligned sizes only)
            nw, rpr, valid, late = _store_form(c)
            assert 1 <= valid <= 4 and nw * rpr <= 64 and 4 * nw <= c.rw + 4 < geo.pitch
            assert c.ini_x >= BORDER                       # the byte before column 0 is a pixel of the row
            align.add(c.ini_x & 3)
            last.add((geo.pitch, valid))
            if late:
                tall.add(geo.pitch)
    assert align == {0, 1, 2, 3}
    assert last == {(p, v) for p in (fc.PITCH_COMPACT, fc.PITCH_WIDE) for v in (1, 2, 3, 4)}, sorted(last)
    assert pitches == tall == {fc.PITCH_COMPACT, fc.PITCH_WIDE}
    assert byte_path == {"w179", "w91"}


@pytest.mark.parametrize("name", NAMES)
def test_planted_arcs_are_corners_of_the_oracle(oracle_mod, name):
    """CPU only: every planted arc has strength iniTh + 1, rests on the ROI's outermost column or row, and is a
    candidate of the oracle's level 0."""
    geo, frames, centres, per = _case(oracle_mod, name)
    img = frames[ARC_FRAME]
    got = {(int(x) + BORDER, int(y) + BORDER) for x, y, _ in per[ARC_FRAME][0][0]}
    assert len(centres) >= 3 * len(geo.levels[0].cells)
    sides = set()
    for x, y in centres:
        assert _strength(img, x, y) == fc.INI_TH + 1, (x, y)
        assert (x, y) in got, (x, y)
        c = fc.cell_of(geo, x, y)
        x0, y0 = c.origin()
        sides |= {s for s, hit in (("left", x - 3 == c.ini_x), ("right", x + 3 == c.ini_x + c.rw - 1),
                                   ("top", y - 3 == c.ini_y), ("bottom", y + 3 == c.ini_y + c.rh - 1)) if hit}
    assert sides == {"left", "right", "top", "bottom"}
    # the edge frames hold both extreme bytes in every cell's outermost columns and rows
    for f in (0, 1):
        for c in geo.levels[0].cells:
            roi = frames[f][c.ini_y:c.ini_y + c.rh, c.ini_x:c.ini_x + c.rw]
            for line in (roi[:, 0], roi[:, -1], roi[0], roi[-1]):
                assert {0, 255} <= set(line.tolist())


def _compare(e, geo, frame, slot, per, what, results=None):
    cands, kps, desc = per[frame]
    for l in range(geo.nlevels):
        g = e.debug_candidates(l, slot)
        if g.tobytes() != cands[l].tobytes():
            pytest.fail("%s: FAST candidates differ, frame %d level %d: %d for the oracle's %d\n%s" % (
                what, frame, l, len(g), len(cands[l]),
                "\n".join(fc.explain(geo, [], frame, l, g, cands[l])) or "the same candidates in another order"))
    gk, gd = results if results is not None else e.results(slot)
    assert len(gk) == len(kps) and gk.tobytes() == kps.tobytes(), (what, "keypoints differ", frame)
    assert gd.tobytes() == desc.tobytes(), (what, "descriptors differ", frame)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_frame_launch_matches_oracle(orbgpu_mod, oracle_mod, name):
    """One frame per launch: one cell per wave."""
    geo, frames, _, per = _case(oracle_mod, name)
    e = orbgpu_mod.BatchExtractor(fc.NFEAT, geo.w, geo.h, 1, nlevels=geo.nlevels, ini_th=fc.INI_TH, min_th=fc.MIN_TH)
    try:
        for f in range(len(frames)):
            e.upload(frames[f][None])
            e.launch()
            e.sync()
            _compare(e, geo, f, 0, per, (name, "one frame"))
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_batch_launch_matches_oracle(orbgpu_mod, oracle_mod, monkeypatch, name):
    """Batches of B = 3 (frames 0..2, then 2..4) through the per-kernel launches: two cells per wave (k_fast_wave)."""
    geo, frames, _, per = _case(oracle_mod, name)
    monkeypatch.setenv("ORBGPU_FLOW", "0")   # read at orb_create
    e = orbgpu_mod.BatchExtractor(fc.NFEAT, geo.w, geo.h, 3, nlevels=geo.nlevels, ini_th=fc.INI_TH, min_th=fc.MIN_TH)
    try:
        for first in (0, 2):
            e.upload(frames[first:first + 3])
            e.launch()
            e.sync()
            for s in range(3):
                _compare(e, geo, first + s, s, per, (name, "B = 3"))
    finally:
        e.close()


FLOW_FAST = 1   # FlowKind (orbgpu_internal.h): resize, fast, octree, describe, chain


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLOW_NAMES)
def test_dataflow_launch_matches_oracle(orbgpu_mod, oracle_mod, monkeypatch, name):
    """The dataflow launch (flow_fast: the same loads at its own cache policy) takes batches of at most two frames:
    frames (0, 1), (2, 3) and (3, 4).  The launch's own task stamps show that its FAST tasks ran in every launch."""
    geo, frames, _, per = _case(oracle_mod, name)
    monkeypatch.setenv("ORBGPU_FLOW", "1")          # read at orb_create
    monkeypatch.setenv("ORBGPU_FLOW_STAMPS", "1")
    monkeypatch.delenv("ORBGPU_FLOW_CHAIN", raising=False)
    monkeypatch.delenv("ORBGPU_FLOW_BLOCKS", raising=False)
    e = orbgpu_mod.BatchExtractor(fc.NFEAT, geo.w, geo.h, 2, nlevels=geo.nlevels, ini_th=fc.INI_TH, min_th=fc.MIN_TH)
    try:
        before = 0
        for first in (0, 2, 3):
            e.upload(frames[first:first + 2])
            e.launch()
            e.sync()
            end = flow_task_ends(orbgpu_mod, e, 2).get(FLOW_FAST, 0)
            assert end > before, (name, first, "the dataflow launch's FAST tasks did not run", before, end)
            before = end
            for s in range(2):
                _compare(e, geo, first + s, s, per, (name, "dataflow launch, B = 2"))
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_host_path_matches_oracle(orbgpu_mod, oracle_mod, name):
    """ORBextractor's operator(): level 0 has rows of a multiple of 64 bytes, so every width takes the format loads."""
    geo, frames, _, per = _case(oracle_mod, name)
    g = orbgpu_mod.ORBextractor(fc.NFEAT, 1.2, geo.nlevels, fc.INI_TH, fc.MIN_TH)
    try:
        for f in range(len(frames)):
            res = g(frames[f])
            _compare(g, geo, f, 0, per, (name, "operator()"), res)
    finally:
        g.close()
