"""k_describe on the planted-decision cases (tests/describe_cases.py; the CPU side is tests/test_describe_cases.py):
every frame through the host path (ORBextractor, one slot per wave) and through BatchExtractor with B = 3 (two slots
per wave: shared pairs, border slots, empty partners), under the default arithmetic, ORB_VARIANT_NO_FMA and
ORB_VARIANT_BLUR_HALFUP, byte for byte against describe_ref under the matching rule and against the oracle under the
matching flag; the frames whose width is no multiple of 4 also from a device buffer with a 64-byte-multiple row
stride and poison in the pad (level 0 is then dword-aligned and takes the interior window form).  Mismatches are
reported by frame, planted keypoint and census items."""
import numpy as np
import pytest

import describe_cases as C
import describe_ref as R
from test_describe_cases import _oracle_run, _ref
from test_gpu_describe_pair import _slot_table

pytestmark = pytest.mark.gpu

BLUR, NOFMA = 4, 8
B = 3
RULES = {0: R.PINNED, NOFMA: R.PINNED._replace(fma=False), BLUR: R.PINNED._replace(blur="halfup")}
FRAMES = C.frames()


def _groups():
    g = {}
    for f in FRAMES:
        g.setdefault((f.img.shape, f.nlevels, f.scale, f.nfeatures), []).append(f)
    out = []
    for fs in g.values():
        for i in range(0, len(fs), B):
            part = fs[i:i + B]
            out.append(part + [fs[0]] * (B - len(part)))   # a short batch is filled with the group's first frame
    return out


GROUPS = _groups()
GROUP_IDS = ["+".join(f.name for f in g) for g in GROUPS]


def _expected(oracle_mod, f, variant):
    ok, od, _, _ = _oracle_run(oracle_mod, f, variant)
    k, d, tr = _ref(oracle_mod, f, RULES[variant])
    assert k.tobytes() == ok.tobytes() and np.array_equal(d, od), f.name   # (the CPU suite's assertion, restated)
    return k, d, tr


def _compare(f, got, exp, where):
    gk, gd = got
    k, d, tr = exp
    names = {(p.level, p.x, p.y): (p.name, p.items) for p in f.plants}
    assert len(gk) == len(k), (where, f.name, len(gk), len(k))
    bad = [(names.get((t.level, t.x, t.y), ("extra", ())), (t.level, t.x, t.y), float(gk[i]["angle"]), float(t.angle),
            np.flatnonzero(np.unpackbits(gd[i] ^ d[i], bitorder="little")).tolist()[:6])
           for i, t in enumerate(tr) if gk[i].tobytes() != k[i].tobytes() or not np.array_equal(gd[i], d[i])]
    assert not bad, (where, f.name, len(bad), bad[:4])


_HOST = {}


@pytest.fixture(scope="module", autouse=True)
def _close_host_extractors():
    yield
    for e in _HOST.values():
        e.close()
    _HOST.clear()


def _host(orbgpu_mod, f, variant):
    key = (f.nfeatures, f.scale, f.nlevels, variant)
    if key not in _HOST:
        _HOST[key] = orbgpu_mod.ORBextractor(f.nfeatures, f.scale, f.nlevels, C.INI_TH, C.MIN_TH, variant=variant)
    return _HOST[key](f.img)


@pytest.mark.parametrize("variant", [0, NOFMA, BLUR])
def test_host_path(orbgpu_mod, oracle_mod, variant):
    for f in FRAMES:
        _compare(f, _host(orbgpu_mod, f, variant), _expected(oracle_mod, f, variant), ("host", variant))


def _batch(orbgpu_mod, oracle_mod, group, variant, stride=None):
    """One context, one launch: per frame (keypoints, descriptors) and the (state, output index) slot table."""
    from orbgpu._lib import check, lib
    f0 = group[0]
    h, w = f0.img.shape
    e = orbgpu_mod.BatchExtractor(f0.nfeatures, w, h, B, scale_factor=f0.scale, nlevels=f0.nlevels, ini_th=C.INI_TH,
                                  min_th=C.MIN_TH, variant=variant)
    d = None
    try:
        if stride is None:
            e.upload(np.stack([f.img for f in group]))
            e.launch()
        else:
            padded = np.full((B, h, stride), 0xA5, np.uint8)   # the pad bytes are never read: any value must do
            padded[:, :, :w] = np.stack([f.img for f in group])
            d = e._alloc(padded.nbytes)
            check(lib().orb_memcpy_h2d(e.h, d, padded.ctypes.data, padded.nbytes), "h2d")
            check(lib().orb_extract_batch_device(e.h, d, B, w, h, stride * h, stride, e.d_kps, e.d_desc, e.d_counts,
                                                 e.kp_cap), "orb_extract_batch_device")
        e.sync()
        res = [e.results(i) for i in range(B)]
        nfeat = oracle_mod.OracleExtractor(f0.nfeatures, f0.scale, f0.nlevels).tables()["n_per_level"]
        tables = []
        for i in range(B):
            levels = []
            for l in range(f0.nlevels):
                lh, lw = e.debug_level_image(l, i).shape
                k = e.debug_level_keypoints(l, i)
                levels.append((lw, lh, k[:, 0].copy(), k[:, 1].copy()))
            aligned0 = (w % 4 == 0) if stride is None else (stride % 4 == 0)
            tables.append(_slot_table(levels, nfeat, aligned0=aligned0, kp_cap=e.kp_cap))
        return res, tables
    finally:
        if d is not None:
            lib().orb_device_free(e.h, d)
        e.close()


def _planted_combos(f, exp, table):
    """(state of slot 0, state of slot 1, which slot) of every planted keypoint of a frame."""
    state, out = table
    at = {(p.level, p.x, p.y) for p in f.plants if not p.name.startswith("filler")}
    seen = set()
    for (s0, s1), (i0, i1) in zip(state, out):
        for slot, i in ((0, i0), (1, i1)):
            if i >= 0:
                t = exp[2][i]
                if (t.level, t.x, t.y) in at:
                    seen.add((int(s0), int(s1), slot))
    return seen


_BATCHES = {}


def _batch_once(orbgpu_mod, oracle_mod, gi, variant):
    """The packed batch of group gi under `variant`, run once per session whichever test asks first."""
    if (gi, variant) not in _BATCHES:
        _BATCHES[(gi, variant)] = _batch(orbgpu_mod, oracle_mod, GROUPS[gi], variant)
    return _BATCHES[(gi, variant)]


@pytest.mark.parametrize("variant", [0, NOFMA, BLUR])
@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=GROUP_IDS)
def test_batch_path(orbgpu_mod, oracle_mod, gi, variant):
    res, _ = _batch_once(orbgpu_mod, oracle_mod, gi, variant)
    for i, f in enumerate(GROUPS[gi]):
        _compare(f, res[i], _expected(oracle_mod, f, variant), ("batch", variant, i))


def test_batch_slot_combinations_among_planted(orbgpu_mod, oracle_mod):
    """Planted keypoints occur as slot 0 and slot 1 of a shared pair (both filled, slot 1 interior), as a border
    slot 1 (not shared), beside an empty slot 1, and as slot 1 beside an empty slot 0 (level 1's first slot is odd)."""
    seen = set()
    for gi, group in enumerate(GROUPS):
        _, tables = _batch_once(orbgpu_mod, oracle_mod, gi, 0)
        for i, f in enumerate(group):
            seen |= _planted_combos(f, _expected(oracle_mod, f, 0), tables[i])
    assert {(2, 2, 0), (2, 2, 1)} <= seen and (1, 2, 0) in seen, sorted(seen)
    assert any(s1 == 1 and slot == 1 for (_, s1, slot) in seen), sorted(seen)
    assert any(s1 == 0 and slot == 0 for (_, s1, slot) in seen), sorted(seen)
    assert any(s0 == 0 and slot == 1 for (s0, _, slot) in seen), sorted(seen)


@pytest.mark.parametrize("variant", [0, NOFMA, BLUR])
@pytest.mark.parametrize("group", [g for g in GROUPS if g[0].img.shape[1] % 4], ids=lambda g: g[0].name)
def test_padded_stride_makes_level0_interior(orbgpu_mod, oracle_mod, group, variant):
    res, tables = _batch(orbgpu_mod, oracle_mod, group, variant, stride=384)
    interior = 0
    for i, f in enumerate(group):
        _compare(f, res[i], _expected(oracle_mod, f, variant), ("padded", variant, i))
        interior += int((tables[i][0] == 2).sum())
    assert interior > 0


def _variant_moves_planted_bits(orbgpu_mod, oracle_mod, variant, carries):
    """On the device, the descriptors of the keypoints planted for a variant's rule differ between the default and
    the variant in the planted bit, and in exactly the bits in which the reference differs under the matching rule."""
    n = 0
    for f in FRAMES:
        plants = [p for p in f.plants if any(carries(i) for i in p.items)]
        if not plants:
            continue
        _, d0 = _host(orbgpu_mod, f, 0)
        _, d1 = _host(orbgpu_mod, f, variant)
        r0, r1 = _expected(oracle_mod, f, 0), _expected(oracle_mod, f, variant)
        idx = {(t.level, t.x, t.y): i for i, t in enumerate(r0[2])}
        for p in plants:
            i = idx[(p.level, p.x, p.y)]
            (bit,) = p.expect["bits"]
            moved = np.flatnonzero(np.unpackbits(d0[i] ^ d1[i], bitorder="little")).tolist()
            want = np.flatnonzero(np.unpackbits(r0[1][i] ^ r1[1][i], bitorder="little")).tolist()
            assert bit in moved and moved == want, (f.name, p.name, bit, moved, want)
            n += 1
    return n


def test_halfup_variant_is_live_on_its_planted_keypoints(orbgpu_mod, oracle_mod):
    """The device's rounding switch: the keypoints planted on an even-quotient tie in the SSE2 body."""
    n = _variant_moves_planted_bits(orbgpu_mod, oracle_mod, BLUR,
                                    lambda it: it == "tie_even_body" or it.startswith("tie_body_w"))
    assert n >= 8


def test_nofma_variant_is_live_on_its_planted_keypoints(orbgpu_mod, oracle_mod):
    """k_describe<false> is not k_describe<true>: the keypoints whose moments put one sample on a different pixel
    under uncontracted offsets."""
    assert _variant_moves_planted_bits(orbgpu_mod, oracle_mod, NOFMA, lambda it: it == "offset_fma") >= 4
