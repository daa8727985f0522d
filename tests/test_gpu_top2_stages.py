"""k_top2_mfma's steady-state stage loop, its last masked stage, the slice merge (k_top2b_merge) and the tie order,
on synthetic descriptor slots with planted structure (tests/top2_cases.py) uploaded in place of an extraction
batch's d_desc / d_counts: orb_hamming_top2_frames_device at three launch shapes whose slices hold several
64-train stages, every output compared exactly with the numpy reference."""
import ctypes

import numpy as np
import pytest

import top2_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(orbgpu_mod):
    # a small extraction context, used only for its handle, device allocations and the stream sync
    bx = orbgpu_mod.BatchExtractor(500, 320, 240, 1)
    yield bx
    bx.close()


def _launch(bx, L, case, d_desc, d_counts, d_out):
    """Prefill the three outputs, run one launch, return (best, idx, second) as (npairs, kp_cap) arrays."""
    from orbgpu import check
    shape = case.shape
    n = shape.npairs * shape.kp_cap
    fill = np.full(n, tc.PREFILL, np.uint32)
    for d in d_out:
        check(L.orb_memcpy_h2d(bx.h, d, fill.ctypes.data, fill.nbytes), "h2d")
    qf, tf = np.ascontiguousarray(case.qf), np.ascontiguousarray(case.tf)
    check(L.orb_hamming_top2_frames_device(bx.h, d_desc, d_counts, shape.kp_cap, shape.npairs,
                                           ctypes.c_void_p(qf.ctypes.data), ctypes.c_void_p(tf.ctypes.data), *d_out),
          "orb_hamming_top2_frames_device")
    bx.sync()
    res = []
    for d in d_out:
        r = np.zeros(n, np.int32)
        check(L.orb_memcpy_d2h(bx.h, r.ctypes.data, d, r.nbytes), "d2h")
        res.append(r.reshape(shape.npairs, shape.kp_cap))
    return res


def _describe(case, plants, p, i):
    """Where a mismatch is: shape, pair, frames and counts, and the plant (class, position, rows) if query i of
    that pair is one."""
    q, t = int(case.qf[p]), int(case.tf[p])
    pl = plants.get((q, t, i))
    what = (f"class {pl.cls}, position {pl.pos} (a, b, c) = ({pl.a}, {pl.b}, {pl.c}), planted {pl.expect}"
            if pl else "background query")
    return (f"shape {case.shape.name}: pair {p} = frames ({q}, {t}) with counts ({case.counts[q]}, "
            f"{case.counts[t]}), query {i}: {what}")


@pytest.mark.parametrize("name", [s.name for s in tc.SHAPES])
def test_top2_stages_slices_and_ties(ctx, name):
    """Every pair of the launch against the reference, exactly: best, first index and second for i < counts[q];
    the prefill untouched for i >= counts[q]; 257 / -1 / 257 where counts[t] == 0 and second 257 where
    counts[t] == 1; a second launch bit-identical."""
    from orbgpu import _lib, check
    L = _lib.lib()
    case, ref = tc.build(name), tc.reference(name)
    shape, cap, counts = case.shape, case.shape.kp_cap, case.counts
    # the launch shape: slices of several stages (tests/test_top2_cases.py holds the table's arithmetic)
    assert L.orb_hamming_top2_slices(shape.npairs, cap, cap) == shape.slices
    assert -(-cap // tc.STAGE) >= (shape.min_stages - 1) * shape.slices + 1
    plants = tc.plant_index(case)
    bx = ctx
    n = shape.npairs * cap
    d_desc, d_counts = bx._alloc(case.desc.nbytes), bx._alloc(counts.nbytes)
    d_out = [bx._alloc(n * 4) for _ in range(3)]
    try:
        check(L.orb_memcpy_h2d(bx.h, d_desc, case.desc.ctypes.data, case.desc.nbytes), "h2d")
        check(L.orb_memcpy_h2d(bx.h, d_counts, counts.ctypes.data, counts.nbytes), "h2d")
        res = _launch(bx, L, case, d_desc, d_counts, d_out)
        again = _launch(bx, L, case, d_desc, d_counts, d_out)
    finally:
        for d in [d_desc, d_counts] + d_out:
            L.orb_device_free(bx.h, d)
    prefill = np.int32(tc.PREFILL)
    names = ("best", "idx", "second")
    seen_empty_q = seen_empty_t = seen_one_t = 0
    for p in range(shape.npairs):
        q, t = int(case.qf[p]), int(case.tf[p])
        nq, nt = int(counts[q]), int(counts[t])
        want = ref[case.combo_of_pair[p]]
        for k in range(3):
            got = res[k][p]
            if not np.array_equal(got[:nq], want[k]):
                i = int(np.flatnonzero(got[:nq] != want[k])[0])
                raise AssertionError(f"{names[k]} {int(got[i])} != {int(want[k][i])} (got "
                                     f"{tuple(int(r[p][i]) for r in res)}, want {tuple(int(w[i]) for w in want)}): "
                                     + _describe(case, plants, p, i))
            if not (got[nq:] == prefill).all():
                i = nq + int(np.flatnonzero(got[nq:] != prefill)[0])
                raise AssertionError(f"{names[k]} written past counts[q] = {nq}: 0x{int(got[i]) & 0xFFFFFFFF:08X} at "
                                     + _describe(case, plants, p, i))
        if nq == 0:
            seen_empty_q += 1
        elif nt == 0:
            seen_empty_t += 1
            assert (res[0][p][:nq] == 257).all() and (res[1][p][:nq] == -1).all() and (res[2][p][:nq] == 257).all(), \
                _describe(case, plants, p, 0)
        elif nt == 1:
            seen_one_t += 1
            assert (res[1][p][:nq] == 0).all() and (res[2][p][:nq] == 257).all(), _describe(case, plants, p, 0)
    assert seen_empty_q and seen_empty_t and seen_one_t
    # every planted query, by its planted triple (the reference was shown to agree without a GPU)
    pairs_of = {}
    for p in range(shape.npairs):
        pairs_of.setdefault((int(case.qf[p]), int(case.tf[p])), []).append(p)
    for pl in case.plants:
        for p in pairs_of[(pl.qframe, pl.tframe)]:
            got = tuple(int(r[p][pl.qi]) for r in res)
            assert got == pl.expect, f"got {got}: " + _describe(case, plants, p, pl.qi)
    for k in range(3):
        assert np.array_equal(again[k], res[k]), f"shape {name}: second launch differs in {names[k]}"
