"""CPU only: the sizes of tests/fast_stage_cases.py hold every staging case, and every plant behaves as designed in
the oracle.  A wrong plant or a size that lost its cell fails here, before any GPU run."""
import numpy as np
import pytest

import fast_stage_cases as fc
import test_gpu_fast_tail as tail


def _host_stride(w):
    return (w + 63) & ~63       # orb_extract's upload pitch (csrc/orbgpu_abi.hip)


def _paths():
    """(size, entry) -> (geometry, level 0 loaded as aligned dwords?): BatchExtractor passes rowStride = width, the
    host path its own 64-byte pitch."""
    out = {}
    for name, (w, h, nlevels) in fc.SIZES.items():
        geo = fc.Geometry(w, h, nlevels)
        out[(name, "batch")] = (geo, geo.level0_aligned(w))
        out[(name, "host")] = (geo, geo.level0_aligned(_host_stride(w)))
    return out


def test_sizes_hold_every_case():
    paths = _paths()

    def cells0(pitch, aligned, entry=None):
        return [c for (name, e), (geo, al) in paths.items() if geo.pitch == pitch and al == aligned
                and entry in (None, e) for c in geo.levels[0].cells]

    # pitch 80, aligned
    wide = cells0(80, True)
    assert {c.B for c in wide} == {0, 1, 2, 3}
    assert {c.nruns for c in wide} >= {3, 4}
    assert any(c.rounds >= 3 and 0 < c.partial < c.rpi for c in wide)
    assert any(c.late for c in wide)
    assert any((c.rw, c.rh, c.dw, c.dh) == (59, 59, 53, 53) and c.nruns == 4 and c.rpi == 16 and c.rounds == 4
               for c in wide)                                    # the largest tile (91 x 91: aligned on the host path)
    # ... and through BatchExtractor alone: every B, three runs, three rounds with a partial last one, late rows
    wide_b = cells0(80, True, "batch")
    assert {c.B for c in wide_b} == {0, 1, 2, 3}
    assert any(c.nruns == 3 and c.rounds == 3 and c.partial == 11 and c.late for c in wide_b)
    # the even form's third store carries the ROI's last column in some cell, for B = 0 and for B = 2
    assert {c.B for c in wide_b if c.last_b3} == {0, 2}
    # pitch 80, per byte: the grid of an aligned size
    g180, g179 = paths[("w180", "batch")], paths[("w179", "batch")]
    assert g180[1] and not g179[1] and g179[0].pitch == 80
    key = lambda c: (c.ci, c.cj, c.ini_x, c.B, c.nruns, c.rpi, c.rpr, c.late, c.dh)   # noqa: E731
    assert [key(c) for c in g179[0].levels[0].cells] == [key(c) for c in g180[0].levels[0].cells]
    assert [c.dw for c in g179[0].levels[0].cells] == [37, 37, 37, 30]
    assert not paths[("w91", "batch")][1] and paths[("w91", "host")][1]   # one frame, both load paths
    # pitch 48, aligned
    geo, al = paths[("w364", "batch")]
    assert al and geo.pitch == 48
    assert {c.B for c in geo.levels[0].cells} == {0, 1, 2, 3}
    assert any(1 <= c.tail <= 3 for c in geo.levels[0].cells)
    assert any(c.late for c in geo.cells())
    assert any(c.last_b3 and c.B == 2 for c in geo.levels[0].cells)
    # pitch 48, per byte: the tail suite's frames (BatchExtractor at an odd width)
    for name, (w, h, nlevels, rows) in tail.SIZES.items():
        assert w % 2 == 1 and fc.Geometry(w, h, nlevels).pitch == 48, name
        ncols, wcell, hcell, cells = tail._grid(w, h)       # the two models agree
        L0 = fc.Geometry(w, h, nlevels).levels[0]
        assert (ncols, wcell, hcell) == (L0.ncols, L0.wcell, L0.hcell)
        assert [(c.ci, c.cj, c.dw, c.dh, c.tail) for c in L0.cells] == cells


@pytest.mark.parametrize("name", list(fc.SIZES))
def test_plants_lie_where_designed(name):
    geo, planted, fr = fc.frames(name)
    assert fr.shape == (fc.NROT + 1, geo.h, geo.w)
    seen = {}
    for r, (img, plants, groups) in enumerate(planted):
        for p in plants:
            c = fc.cell_of(geo, p.x, p.y)
            assert c is p.cell and groups[(c.ci, c.cj)] == p.group, p
            rnd, run, late = c.where(p.ox, p.oy)
            for k, v in p.want.items():
                if k != "seam":
                    assert {"round": rnd, "run": run, "late": late}[k] == v, (p, k, rnd, run, late)
            if p.carrier == "p4":      # column +3 lies in the next window / run / past the domain
                far = p.ox + 3
                assert {"window": far // 8 > p.ox // 8, "run": far // 16 > p.ox // 16,
                        "domain": far >= c.dw - 1 and far < c.rw - 3}[p.want["seam"]], p
            if p.carrier == "p12":
                far = p.ox - 3
                assert {"window": far // 8 < p.ox // 8, "run": far // 16 < p.ox // 16}[p.want["seam"]], p
            seen.setdefault((c.ci, c.cj), set()).add((p.group, p.name.split(",")[0]))
    for c in geo.levels[0].cells:      # every cell holds every group once over the rotations
        have = seen[(c.ci, c.cj)]
        assert {g for g, _ in have} >= set(fc.GROUPS) - {"seamB"}, (c.ci, c.cj)   # (seamB: seamA's overflow)
        names = {n for _, n in have}
        for k in range(1, c.rounds):
            assert {"last row of round %d" % (k - 1), "first row of round %d" % k} <= names, (c.ci, c.cj, k)
        if c.late and 8 * c.rpr - 3 < c.dh:
            assert {"last prefetched row", "first late row", "weak"} <= names
        xs = {x for x in (7, 8, 15, 16, 31, 32, 47, 48) if x < c.dw - 4} | {c.dw - 1, c.dw - 2, c.dw - 4}
        got = {p.ox for _, ps, _ in planted for p in ps if p.cell is c and p.carrier and p.kept}
        assert xs <= got, (c.ci, c.cj, sorted(xs - got))
        for side in ("p4", "p12"):     # bright and dark on each side
            pol = {"bright" in p.name for _, ps, _ in planted for p in ps if p.cell is c and p.carrier == side}
            assert pol == {True, False} or (side == "p12" and c.dw <= 16), (c.ci, c.cj, side)


@pytest.mark.parametrize("name", list(fc.SIZES))
def test_plants_behave_as_designed_in_the_oracle(oracle_mod, name):
    geo, planted, fr, per = fc.expected(oracle_mod, name)
    for r, (img, plants, groups) in enumerate(planted):
        assert np.array_equal(fr[r], img)
        found = {(int(x) + fc.BORDER, int(y) + fc.BORDER): int(s) for x, y, s in per[r][0][0]}
        for p in plants:
            assert fc._strength(img, p.x, p.y) == p.m, (p, "the plant does not have its arc strength")
            if p.kept:
                assert found.get((p.x, p.y)) == p.m - 1, (p, "the oracle does not keep the planted corner")
            else:
                assert (p.x, p.y) not in found, (p, "the oracle keeps a planted non-corner")
            if p.carrier:      # exactly one pixel of each compass pair passes, the carrier among them
                v = int(img[p.y, p.x])
                ring = [int(img[p.y + dy, p.x + dx]) for dx, dy in fc.CIRCLE]
                t = p.m - 1        # the threshold the centre just passes (the twin: its own strength - 1)
                ok = [abs(ring[i] - v) > t for i in (0, 4, 8, 12)]
                assert ok[0] != ok[2] and ok[1] != ok[3] and ok[{"p4": 1, "p12": 3}[p.carrier]], p
        assert len(found) == sum(p.kept for p in plants), (name, r, "the oracle keeps something that is no plant")
        for c in geo.levels[0].cells:      # the cells of the second pass
            group = groups[(c.ci, c.cj)]
            if group not in ("weak", "plateau"):
                continue
            roi = np.ascontiguousarray(img[c.ini_y:c.ini_y + c.rh, c.ini_x:c.ini_x + c.rw])
            mine = [p for p in plants if p.cell is c]
            assert len(oracle_mod.fast_roi(roi, fc.INI_TH)) == 0, (name, r, c.ci, c.cj)
            weak = {(int(x), int(y)) for x, y, s in oracle_mod.fast_roi(roi, fc.MIN_TH)}
            assert weak == {(p.ox + 3, p.oy + 3) for p in mine if p.kept}, (name, r, c.ci, c.cj)
            if group == "plateau":         # corners at iniTh on their own, adjacent and equal: only the NMS drops them
                pairs = [p for p in mine if p.name.startswith("equal")]
                assert len(pairs) == 4 and all(p.m > fc.INI_TH and not p.kept for p in pairs)
                for a, b in (pairs[:2], pairs[2:]):
                    assert a.m == b.m and abs(a.x - b.x) + abs(a.y - b.y) == 1
                if c.rounds > 1 and c.dh > c.rpi + 7:
                    assert {p.oy // c.rpi for p in pairs} >= {0, 1}, (name, c.ci, c.cj)
            elif c.rounds > 1:
                assert {p.oy // c.rpi for p in mine if p.kept} >= {0, 1}, (name, c.ci, c.cj)
    # the noise frame: more corners than one 64-entry chunk of the in-place compaction in some cell
    dense = {}
    img = fr[-1]
    for c in geo.levels[0].cells:
        roi = np.ascontiguousarray(img[c.ini_y:c.ini_y + c.rh, c.ini_x:c.ini_x + c.rw])
        dense[(c.ci, c.cj)] = len(oracle_mod.fast_roi(roi, fc.INI_TH))
    assert max(dense.values()) > 64, dense


def test_bench_geometries_tile_pitch():
    """The tile pitch of the BASELINE configurations: 640 x 480 at 8 levels is not compact (level 7 is 179 x 134,
    147 px over 4 columns: cells 37 wide), 1280 x 720 is."""
    pitch = {cfg: fc.Geometry(w, h, 8).pitch for cfg, (w, h) in fc.BENCH_SIZES.items()}
    assert pitch == {"C1": 80, "C2": 80, "C3": 48, "C4": 48, "C5": 48}
    g = fc.Geometry(640, 480, 8)
    assert [L.wcell for L in g.levels] == [31, 32, 32, 31, 31, 33, 31, 37]
    assert max(L.wcell for L in fc.Geometry(1280, 720, 8).levels) == 33
    assert fc.Geometry(320, 240, 8).pitch == 80          # the arc suite's frame (level 7: one cell 57 wide)
