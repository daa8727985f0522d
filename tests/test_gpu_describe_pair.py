"""k_describe's paired composition: a wave's two keypoint slots share one orientation-trig pass.

The paired form runs only with two or more frames in a batch (two slots per wave), so every case goes through
BatchExtractor with B = 3 and is compared with the oracle byte for byte.  A wave owns slots (2i, 2i + 1) of the
frame's slot table, where level l's keypoint k sits in slot kp_base[l] + k; the pair is shared when both slots hold
a keypoint and slot 2i + 1's window is interior.  The tests read the level keypoints back from the device, work out
each wave's combination (interior / border / empty per slot) and assert that the inputs contain every combination
they claim to cover, and that some shared pair holds two angles on different branches of fastAtan2 and sincosf.
(No keypoint of these inputs has a flat patch, m01 = m10 = 0: a FAST corner's patch is never symmetric.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOFMA = 8
B = 3
PI4_TOP12 = 0x3F4   # abstop12(0x1.921FB6p-1f): glibc's |x| < pi/4 test compares the top 12 bits


def _frames(w, h, kind, first):
    from orbgpu.synth import synth_batch
    return synth_batch(w, h, B, first=first, kind=kind)


_ORACLE = {}


def _oracle(oracle_mod, w, h, kind, first, nf, variant):
    """The oracle's (keypoints, descriptors) of every frame of a case, computed once and shared (never modified)."""
    key = (w, h, kind, first, nf, variant)
    if key not in _ORACLE:
        o = oracle_mod.OracleExtractor(nf, flags=variant)
        _ORACLE[key] = [o(f) for f in _frames(w, h, kind, first)]
    return _ORACLE[key]


def _run(orbgpu_mod, w, h, kind, first, nf, variant, launches=1):
    """One context: the batch extracted `launches` times; per launch (counts, [(kps, desc) per frame]), then the
    slot table of every frame, per level (w, h, x[], y[]) read back from the device, and the table's length."""
    e = orbgpu_mod.BatchExtractor(nf, w, h, B, variant=variant)
    e.upload(_frames(w, h, kind, first))
    runs = []
    for _ in range(launches):
        e.launch()
        e.sync()
        runs.append((e.counts().copy(), [e.results(f) for f in range(B)]))
    levels = []
    for f in range(B):
        per = []
        for l in range(8):
            lh, lw = e.debug_level_image(l, f).shape
            k = e.debug_level_keypoints(l, f)
            per.append((lw, lh, k[:, 0].copy(), k[:, 1].copy()))
        levels.append(per)
    kp_cap = e.kp_cap
    e.close()
    return runs, levels, kp_cap


def _slot_table(levels, nfeat, aligned0, kp_cap):
    """state per slot of a frame: 0 empty, 1 border, 2 interior (extract_kernels.hip desc_slot), and the output
    index of each filled slot; the slot layout is orbgpu_abi.hip's (kp_cap, kp_base)."""
    state, out = [], []
    n_out = 0
    for l, (w, h, x, y) in enumerate(levels):
        n_ini = int(np.round(np.float32(w - 32) / np.float32(h - 32)))
        cap = max(int(nfeat[l]) + 3, 4 * n_ini) + 4
        assert len(x) <= cap
        aligned = aligned0 if l == 0 else True
        inter = aligned & (x >= 21) & (x + 27 <= w) & (y >= 21) & (y + 21 < h)
        st = np.zeros(cap, np.int32)
        st[:len(x)] = np.where(inter, 2, 1)
        ix = np.full(cap, -1, np.int32)
        ix[:len(x)] = n_out + np.arange(len(x))
        n_out += len(x)
        state.append(st)
        out.append(ix)
    state, out = np.concatenate(state), np.concatenate(out)
    assert len(state) == kp_cap, (len(state), kp_cap)   # the layout restated here is the device's
    if len(state) & 1:
        state, out = np.append(state, 0), np.append(out, -1)
    return state.reshape(-1, 2), out.reshape(-1, 2)


def _branches(angle):
    """(sincosf branch, quadrant, fastAtan2 side) of an angle in degrees, None where it is within 1 degree of a
    boundary between two branches (the classification needs no exact boundary: the assertions want clear cases)."""
    a = float(angle)
    if min(abs(a % 45.0), 45.0 - abs(a % 45.0)) < 1.0:
        return None
    rad = np.float32(np.float32(a) * np.float32(np.pi / 180.0))
    small = ((int(rad.view(np.uint32)) >> 20) & 0x7FF) < PI4_TOP12
    quad = int(np.floor(a / 90.0 + 0.5)) & 3
    side = (a % 180.0) < 45.0 or (a % 180.0) > 135.0   # |x| >= |y|
    return small, quad, side


def _combos(state):
    return {(int(a), int(b)) for a, b in state}


def _check_case(orbgpu_mod, oracle_mod, w, h, kind, first, nf, variant):
    ref = _oracle(oracle_mod, w, h, kind, first, nf, variant)
    runs, levels, kp_cap = _run(orbgpu_mod, w, h, kind, first, nf, variant)
    counts, res = runs[0]
    for f in range(B):
        gk, gd = res[f]
        ok, od = ref[f]
        assert counts[f] == len(ok), (f, counts[f], len(ok))
        assert gk.tobytes() == ok.tobytes() and np.array_equal(gd, od), f
    nfeat = oracle_mod.OracleExtractor(nf).tables()["n_per_level"]
    tables = [_slot_table(levels[f], nfeat, aligned0=(w % 4 == 0), kp_cap=kp_cap) for f in range(B)]
    return ref, tables, levels


# (w, h, kind, first frame, nfeatures)
CASES = [
    (320, 240, "scene", 0, 500),
    (320, 240, "noise", 3, 100),
    (320, 240, "scene", 6, 333),
]


@pytest.mark.parametrize("variant", [0, NOFMA])
@pytest.mark.parametrize("w,h,kind,first,nf", CASES)
def test_pair_matches_oracle(orbgpu_mod, oracle_mod, w, h, kind, first, nf, variant):
    _check_case(orbgpu_mod, oracle_mod, w, h, kind, first, nf, variant)


def test_pair_slot_combinations_occur(orbgpu_mod, oracle_mod):
    """Every combination of (slot 0, slot 1) in {interior, border} and both orders of an empty partner occur in
    the inputs of CASES, some level's count is odd, and some wave straddles a level boundary (slot 0 the last slot
    of a level's table, slot 1 the first keypoint of the next level)."""
    seen, odd, straddle = set(), False, False
    for (w, h, kind, first, nf) in CASES:
        _, tables, levels = _check_case(orbgpu_mod, oracle_mod, w, h, kind, first, nf, 0)
        nfeat = oracle_mod.OracleExtractor(nf).tables()["n_per_level"]
        for f in range(B):
            state, _ = tables[f]
            seen |= _combos(state)
            odd |= any(len(x) & 1 for (_, _, x, _) in levels[f])
            base = 0
            for l, (lw, lh, x, _) in enumerate(levels[f][:-1]):
                n_ini = int(np.round(np.float32(lw - 32) / np.float32(lh - 32)))
                base += max(int(nfeat[l]) + 3, 4 * n_ini) + 4
                # the next level starts on an odd slot: its first keypoint is some wave's slot 1
                straddle |= bool(base & 1) and len(levels[f][l + 1][2]) > 0
    for combo in [(2, 2), (2, 1), (1, 2), (1, 1), (2, 0), (1, 0), (0, 2), (0, 1)]:
        assert combo in seen, (combo, sorted(seen))
    assert odd and straddle, (odd, straddle)


def test_pair_angles_on_different_branches(orbgpu_mod, oracle_mod):
    """Some shared pair (both slots filled, slot 1 interior) holds two angles that take different branches: sincosf
    below / above pi/4, different quadrants of the reduction, and the two sides of fastAtan2's |x| >= |y|."""
    diff_small = diff_quad = diff_side = 0
    for (w, h, kind, first, nf) in CASES:
        ref, tables, _ = _check_case(orbgpu_mod, oracle_mod, w, h, kind, first, nf, 0)
        for f in range(B):
            state, out = tables[f]
            ang = ref[f][0]["angle"]
            for (s0, s1), (i0, i1) in zip(state, out):
                if s0 == 0 or s1 != 2:
                    continue
                b0, b1 = _branches(ang[i0]), _branches(ang[i1])
                if b0 is None or b1 is None:
                    continue
                diff_small += b0[0] != b1[0]
                diff_quad += (not b0[0]) and (not b1[0]) and b0[1] != b1[1]
                diff_side += b0[2] != b1[2]
    assert diff_small > 0 and diff_quad > 0 and diff_side > 0, (diff_small, diff_quad, diff_side)


@pytest.mark.parametrize("variant", [0, NOFMA])
def test_pair_deterministic(orbgpu_mod, oracle_mod, variant):
    """The same batch three times in one context and once in a second one: counts, keypoints and descriptors are
    byte-equal across all four runs (and equal the oracle's)."""
    w, h, kind, first, nf = CASES[0]
    ref = _oracle(oracle_mod, w, h, kind, first, nf, variant)
    runs = _run(orbgpu_mod, w, h, kind, first, nf, variant, launches=3)[0]
    runs += _run(orbgpu_mod, w, h, kind, first, nf, variant)[0]
    c0, r0 = runs[0]
    for f in range(B):
        assert r0[f][0].tobytes() == ref[f][0].tobytes() and np.array_equal(r0[f][1], ref[f][1]), f
    for i, (c, r) in enumerate(runs[1:], 1):
        assert c.tobytes() == c0.tobytes(), i
        for f in range(B):
            assert r[f][0].tobytes() == r0[f][0].tobytes() and r[f][1].tobytes() == r0[f][1].tobytes(), (i, f)


@pytest.mark.parametrize("variant", [0, NOFMA])
def test_pair_odd_frame_size(orbgpu_mod, oracle_mod, variant):
    """641 x 479: blur tail columns (samples at x >= w & ~3 round half-up) together with pairing; level 0's rows
    are not dword-aligned there, so its keypoints all take the border form (slot 1 on the border: not shared)."""
    _, tables, _ = _check_case(orbgpu_mod, oracle_mod, 641, 479, "scene", 2, 1000, variant)
    seen = set()
    for state, _ in tables:
        seen |= _combos(state)
    assert (2, 2) in seen and (1, 2) in seen and (1, 1) in seen, sorted(seen)
