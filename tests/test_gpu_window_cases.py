"""GPU parity of the window matchers with tests/window_ref.py on the planted case of tests/window_cases.py:
SearchForInitialization and BirdviewMatch over candidate lists (k_topk), the same lists reversed (the expected answer
recomputed by the reference), and the grid form, where k_window_topk does Frame::GetFeaturesInArea itself over F2's
grid.  tests/test_window_cases.py checks on the CPU that the case realises the decisions it is named for."""
import numpy as np
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu


def _report(got_n, got, want_n, want):
    c = wc.case()
    bad = np.flatnonzero(got != want).tolist()
    items = sorted({p.item for p in c.plants if p.i1 in bad})
    regions = sorted({c.region1[i] for i in bad})
    return [] if got_n == want_n and not bad else [(got_n, want_n, items, regions, bad[:8], got[bad[:8]].tolist(),
                                                   want[bad[:8]].tolist())]


@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("level0_only", (True, False))
def test_list_form_matches_reference(orbgpu_mod, level0_only, reverse):
    c = wc.case()
    m = orbgpu_mod.ORBmatcher(wc.NNRATIO, True)
    off, idx = wc.csr(wc.candidates(reverse))
    fn = m.SearchForInitialization if level0_only else m.BirdviewMatch
    n, got = fn(c.desc1, c.kps1, c.desc2, c.kps2, off, idx)
    want_n, want, _ = wc.expected(level0_only, reverse)
    assert not _report(n, got, want_n, want)


@pytest.mark.parametrize("level0_only", (True, False))
def test_grid_form_matches_reference(orbgpu_mod, level0_only):
    c = wc.case()
    m = orbgpu_mod.ORBmatcher(wc.NNRATIO, True)
    grid = wc.grid().csr()
    mine = orbgpu_mod.frame_grid(c.kps2, *wc.BOUNDS)
    assert mine[:2] == grid[:2] and np.array_equal(mine[2], grid[2]) and np.array_equal(mine[3], grid[3])
    n, got = m.window_match_grid(level0_only, c.desc1, c.kps1, c.desc2, c.kps2, grid=grid, window=wc.R,
                                 min_xy=(wc.BOUNDS[0], wc.BOUNDS[2]))
    want_n, want, _ = wc.expected(level0_only)
    assert not _report(n, got, want_n, want)
    # the window centres given explicitly (vbPrevMatched at its initial value): the same answer
    cen = np.stack([c.kps1["x"], c.kps1["y"]], 1).astype(np.float32)
    n, got = m.window_match_grid(level0_only, c.desc1, c.kps1, c.desc2, c.kps2, grid=grid, window=wc.R, centres=cen,
                                 min_xy=(wc.BOUNDS[0], wc.BOUNDS[2]))
    assert not _report(n, got, want_n, want)
