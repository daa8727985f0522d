"""GPU: the batched birdview stream (orb_bird_extract_batch / orb_bird_extract_batch_device) against
oracle.OracleCvORB(nf).extract(img, mask) per frame and against the single call on the same object, byte for byte."""
import ctypes

import numpy as np
import pytest

import bird_batch_cases as bc

pytestmark = pytest.mark.gpu

NF = 500                      # nfeatures of the 200x150 .. 323x241 cases (300 at 200x150)
MAX_BATCH = 64                # ORB_BIRD_MAX_BATCH
ERR_ARG, ERR_CAPACITY = -1, -3


@pytest.fixture(scope="module")
def bird(orbgpu_mod):
    b = orbgpu_mod.BirdORB(NF)
    yield b
    b.close()


def _check(results, nf, frames, mask_ids, what):
    assert len(results) == len(frames)
    for f, (fr, mi) in enumerate(zip(frames, mask_ids)):
        bc.assert_frame(results[f], nf, fr, mi, f"{what}: frame {f} {fr} mask {mi}")


def _masks_arg(frames, mask_ids):
    """mask_ids: all None, all one index (shared), or one index per frame."""
    if all(m is None for m in mask_ids):
        return None
    w, h = frames[0][:2]
    if len(set(mask_ids)) == 1 and len(mask_ids) > 1:
        return bc.mask(w, h, mask_ids[0]).copy()
    return [bc.mask(w, h, m).copy() for m in mask_ids]


def _run_host(bird, frames, mask_ids):
    ms = _masks_arg(frames, mask_ids)
    keep = None if ms is None else ([m.copy() for m in ms] if isinstance(ms, list) else ms.copy())
    out = bird.extract_batch([bc.frame(*fr) for fr in frames], ms)
    if isinstance(ms, list):   # the caller's masks are unchanged
        assert all(np.array_equal(a, b) for a, b in zip(ms, keep))
    elif ms is not None:
        assert np.array_equal(ms, keep)
    return out


def _device_pack(arrays, stride, pitch):
    """arrays of one (h, w) shape at `stride` bytes per row, `pitch` bytes per frame, poison between."""
    h, w = arrays[0].shape
    buf = np.full(len(arrays) * pitch + stride, 0xA5, np.uint8)
    for f, a in enumerate(arrays):
        rows = np.lib.stride_tricks.as_strided(buf[f * pitch:], (h, w), (stride, 1))
        rows[:] = a
    return buf


def _run_device(bird, frames, mask_ids, pad=False, cap=None):
    import torch
    w, h = frames[0][:2]
    stride = w + 13 if pad else w
    pitch = stride * h + (101 if pad else 0)
    hi = _device_pack([bc.frame(*fr) for fr in frames], stride, pitch)
    di = torch.from_numpy(hi).cuda()
    dm, hm, mpitch = None, None, 0
    if not all(m is None for m in mask_ids):
        shared = len(set(mask_ids)) == 1 and len(mask_ids) > 1
        ids = mask_ids[:1] if shared else mask_ids
        hm = _device_pack([bc.mask(w, h, m) for m in ids], stride, pitch)
        dm = torch.from_numpy(hm).cuda()
        mpitch = 0 if shared else pitch
    torch.cuda.synchronize()
    out = bird.extract_batch_device(di.data_ptr(), len(frames), w, h, frame_pitch=pitch,
                                    d_masks=None if dm is None else dm.data_ptr(), mask_frame_pitch=mpitch, cap=cap,
                                    stride=stride, mask_stride=stride)
    # the caller's device images and masks are only read
    assert np.array_equal(di.cpu().numpy(), hi)
    if dm is not None:
        assert np.array_equal(dm.cpu().numpy(), hm)
    return out


# ---------------------------------------------------------------- batch sizes
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_batch_sizes(bird, B):
    frames = bc.FIVE[:B] if B < 5 else bc.FIVE
    ids = [fr[2] for fr in frames]
    _check(_run_device(bird, frames, ids), NF, frames, ids, f"B={B}")


def test_batch_of_five_forward_and_reverse(bird):
    """Every frame's result is its own: a wave that reads another frame's pyramid, level-0 image or blurred
    pyramid shows as a mismatch named by frame index."""
    assert [fr[3] for fr in bc.FIVE] == ["scene", "scene", "flat", "scene", "noise"]
    ids = [fr[2] for fr in bc.FIVE]
    _check(_run_device(bird, bc.FIVE, ids), NF, bc.FIVE, ids, "forward")
    rev = bc.FIVE[::-1]
    _check(_run_device(bird, rev, ids[::-1]), NF, rev, ids[::-1], "reverse")
    # flat frame: nothing; the other four: distinct results
    assert len(bc.expected(NF, bc.FIVE[2], 10)[0]) == 0
    assert len({bc.expected(NF, fr, fr[2])[0].tobytes() for fr in bc.FIVE}) == 5


def test_issue_table_counts():
    """The frames of the suite as the oracle sees them on the CPU; the oracle itself culls at least one point
    after cornerSubPix in some frame, so the keep compaction is exercised."""
    table = [(300, (200, 150, 6, "scene"), 6, 184), (300, (200, 150, 6, "scene"), None, 219),
             (500, (320, 240, 7, "scene"), 7, 452), (500, (323, 241, 9, "scene"), 9, 457),
             (500, (320, 240, 8, "noise"), None, 453), (500, (320, 240, 10, "flat"), 10, 0),
             (2000, (640, 480, 12, "scene"), 12, 2000), (2000, (640, 480, 3, "noise"), None, 1964)]
    for nf, fr, mi, n in table:
        assert len(bc.expected(nf, fr, mi)[0]) == n, (fr, mi)
    assert bc.detected(500, (320, 240, 8, "noise"), None) == 454
    assert bc.detected(2000, (640, 480, 3, "noise"), None) == 1966


# ---------------------------------------------------------------- masks
@pytest.mark.parametrize("mode", ["none", "shared", "per_frame"])
def test_mask_modes(bird, mode):
    frames = bc.FIVE
    ids = {"none": [None] * 5, "shared": [7] * 5, "per_frame": [fr[2] for fr in frames]}[mode]
    _check(_run_device(bird, frames, ids), NF, frames, ids, mode)
    _check(_run_host(bird, frames, ids), NF, frames, ids, mode + " (host form)")


def test_identical_images_different_masks_and_shared_mask(bird):
    a, b = bc.FIVE[0], bc.FIVE[1]
    two = [a, a]
    _check(_run_device(bird, two, [7, 11]), NF, two, [7, 11], "one image, two masks")
    assert bc.expected(NF, a, 7)[0].tobytes() != bc.expected(NF, a, 11)[0].tobytes()
    _check(_run_device(bird, [a, b], [11, 11]), NF, [a, b], [11, 11], "two images, shared mask")
    _check(_run_host(bird, [a, b], [11, 11]), NF, [a, b], [11, 11], "two images, shared mask (host form)")


# ---------------------------------------------------------------- strides
@pytest.mark.parametrize("w,h,nf,idxs", [(320, 240, 500, (7, 11, 13)), (323, 241, 500, (9, 4)), (200, 150, 300, (6, 2, 5))])
@pytest.mark.parametrize("masked", [True, False])
def test_padded_input(orbgpu_mod, w, h, nf, idxs, masked):
    frames = [(w, h, i, "scene") for i in idxs]
    ids = list(idxs) if masked else [None] * len(idxs)
    b = orbgpu_mod.BirdORB(nf)
    try:
        _check(_run_device(b, frames, ids, pad=True), nf, frames, ids, f"padded {w}x{h}")
        if masked:   # padded shared mask
            sh = [idxs[0]] * len(idxs)
            _check(_run_device(b, frames, sh, pad=True), nf, frames, sh, f"padded {w}x{h}, shared mask")
    finally:
        b.close()


# ---------------------------------------------------------------- second download
def test_second_candidate_download(orbgpu_mod):
    """640x480: the noise frame has 55,495 candidates, above the 16,384 speculative prefix; the scene frame
    fits.  Both orders, so the frame that needs the second download is first and last."""
    scene, noise = (640, 480, 12, "scene"), (640, 480, 3, "noise")
    b = orbgpu_mod.BirdORB(2000)
    try:
        # a fresh object starts from the 16,384 prefix: the second frame needs the second download
        _check(_run_host(b, [scene, noise], [None, None]), 2000, [scene, noise], [None, None], "scene, noise")
    finally:
        b.close()
    b = orbgpu_mod.BirdORB(2000)
    try:
        _check(_run_device(b, [noise, scene], [None, None]), 2000, [noise, scene], [None, None], "noise, scene")
        # the prefix has grown to the noise frame's count: the same batch again takes one download
        _check(_run_device(b, [noise, scene], [None, None]), 2000, [noise, scene], [None, None], "again")
    finally:
        b.close()
    # the oracle culls points after cornerSubPix in the noise frame: the keep compaction is exercised
    assert bc.detected(2000, noise, None) > len(bc.expected(2000, noise, None)[0])
    # points culled after cornerSubPix in the noise frame, none in the masked scene frame's 2,000
    assert bc.detected(2000, noise, None) - len(bc.expected(2000, noise, None)[0]) == 2


# ---------------------------------------------------------------- reuse of one object
def test_reuse_one_object(orbgpu_mod):
    big = (640, 480, 12, "scene")
    b = orbgpu_mod.BirdORB(NF)
    try:
        ids = [fr[2] for fr in bc.FIVE]
        _check(_run_device(b, bc.FIVE[:2], ids[:2]), NF, bc.FIVE[:2], ids[:2], "B=2")
        _check(_run_device(b, bc.FIVE, ids), NF, bc.FIVE, ids, "B=5")
        fr = bc.FIVE[3]
        bc.assert_frame(b.extract(bc.frame(*fr), bc.mask(320, 240, 13).copy()), NF, fr, 13, "single extract")
        _check(_run_device(b, [big], [12]), NF, [big], [12], "B=1 at 640x480")
        _check(_run_device(b, bc.FIVE[2:], ids[2:]), NF, bc.FIVE[2:], ids[2:], "B=3")
        # the single call on the same object agrees frame by frame
        for f, fr in enumerate(bc.FIVE):
            kg, dg = b.extract(bc.frame(*fr), bc.mask(320, 240, fr[2]).copy())
            bc.assert_frame((kg, dg), NF, fr, fr[2], f"single call, frame {f}")
    finally:
        b.close()


# ---------------------------------------------------------------- raw C-ABI: capacity and edge arguments
def _raw_device(orbgpu_mod, bird, frames, mask_ids, n, cap, frame_pitch=None, poison=0xCD):
    """orb_bird_extract_batch_device on poisoned outputs -> (status, kps, desc, counts)."""
    import torch
    from orbgpu import KP_DTYPE
    from orbgpu._lib import lib
    w, h = frames[0][:2]
    di = torch.from_numpy(np.stack([bc.frame(*fr) for fr in frames])).cuda()
    dm = None
    if mask_ids is not None:
        dm = torch.from_numpy(np.stack([bc.mask(w, h, m) for m in mask_ids])).cuda()
    torch.cuda.synchronize()
    rows = max(len(frames), 1)
    kps = np.frombuffer(bytes([poison]) * (rows * max(cap, 1) * KP_DTYPE.itemsize), KP_DTYPE).copy()
    desc = np.full((rows * max(cap, 1), 32), poison, np.uint8)
    counts = np.full(max(rows, n, 1), -77, np.int32)
    st = lib().orb_bird_extract_batch_device(
        bird.h, n, ctypes.c_void_p(di.data_ptr()), w, h, w, w * h if frame_pitch is None else frame_pitch,
        None if dm is None else ctypes.c_void_p(dm.data_ptr()), w, w * h if dm is not None else 0,
        kps.ctypes.data_as(ctypes.c_void_p), desc.ctypes.data_as(ctypes.c_void_p), cap,
        counts.ctypes.data_as(ctypes.c_void_p))
    return st, kps.reshape(rows, -1), desc.reshape(rows, -1, 32), counts


def _poisoned(a, poison=0xCD):
    return bool((np.ascontiguousarray(a).view(np.uint8) == poison).all())


def test_capacity(orbgpu_mod, bird):
    frames, ids = bc.FIVE, [fr[2] for fr in bc.FIVE]
    want = [len(bc.expected(NF, fr, mi)[0]) for fr, mi in zip(frames, ids)]
    cap = sorted(want)[-2]
    assert cap < max(want) and want.count(max(want)) == 1
    st, kps, desc, counts = _raw_device(orbgpu_mod, bird, frames, ids, 5, cap)
    assert st == ERR_CAPACITY
    assert counts[:5].tolist() == want
    for f, (fr, mi) in enumerate(zip(frames, ids)):
        n = want[f]
        if n > cap:   # the frame that does not fit is left at its poison value
            assert _poisoned(kps[f]) and _poisoned(desc[f]), f
            continue
        bc.assert_frame((kps[f, :n], desc[f, :n]), NF, fr, mi, f"capacity: frame {f}")
        assert _poisoned(kps[f, n:]) and _poisoned(desc[f, n:]), f   # slots past the count keep their poison
    # with room for all, the same call succeeds
    st, kps, desc, counts = _raw_device(orbgpu_mod, bird, frames, ids, 5, max(want))
    assert st == 0 and counts[:5].tolist() == want
    for f, (fr, mi) in enumerate(zip(frames, ids)):
        bc.assert_frame((kps[f, :want[f]], desc[f, :want[f]]), NF, fr, mi, f"full capacity: frame {f}")
        assert _poisoned(kps[f, want[f]:]) and _poisoned(desc[f, want[f]:]), f


def test_edge_arguments(orbgpu_mod, bird):
    from orbgpu._lib import lib
    frames, ids = bc.FIVE, [fr[2] for fr in bc.FIVE]

    def untouched(r):
        st, kps, desc, counts = r
        return _poisoned(kps) and _poisoned(desc) and (counts == -77).all()

    r = _raw_device(orbgpu_mod, bird, frames, ids, 0, 600)              # nframes = 0: a no-op
    assert r[0] == 0 and untouched(r)
    r = _raw_device(orbgpu_mod, bird, frames, ids, MAX_BATCH + 1, 600)
    assert r[0] == ERR_ARG and untouched(r)
    r = _raw_device(orbgpu_mod, bird, frames, ids, -1, 600)
    assert r[0] == ERR_ARG and untouched(r)
    r = _raw_device(orbgpu_mod, bird, frames, ids, 5, 600, frame_pitch=320 * 240 - 1)   # short frame_pitch
    assert r[0] == ERR_ARG and untouched(r)
    # three masks for five frames (host form)
    from orbgpu import KP_DTYPE
    imgs = [bc.frame(*fr) for fr in frames]
    ms = [bc.mask(320, 240, i) for i in ids[:3]]
    ip = (ctypes.c_void_p * 5)(*[i.ctypes.data for i in imgs])
    mp = (ctypes.c_void_p * 3)(*[m.ctypes.data for m in ms])
    kps = np.frombuffer(b"\xCD" * (5 * 600 * KP_DTYPE.itemsize), KP_DTYPE).copy()
    desc = np.full((5 * 600, 32), 0xCD, np.uint8)
    counts = np.full(5, -77, np.int32)
    args = (kps.ctypes.data_as(ctypes.c_void_p), desc.ctypes.data_as(ctypes.c_void_p), 600,
            counts.ctypes.data_as(ctypes.c_void_p))
    assert lib().orb_bird_extract_batch(bird.h, 5, ip, 320, 240, 320, mp, 3, 320, *args) == ERR_ARG
    assert _poisoned(kps) and _poisoned(desc) and (counts == -77).all()
    assert lib().orb_bird_extract_batch(bird.h, 5, ip, 320, 240, 320, mp, 3, 320, args[0], args[1], 600, None) == ERR_ARG
    # a zero-sized image gives all counts 0
    assert lib().orb_bird_extract_batch(bird.h, 5, ip, 0, 240, 320, None, 0, 0, *args) == 0
    assert (counts == 0).all() and _poisoned(kps) and _poisoned(desc)
    empty = bird.extract_batch([np.zeros((0, 0), np.uint8)] * 3)
    assert len(empty) == 3 and all(len(k) == 0 and d.shape == (0, 32) for k, d in empty)
    assert bird.extract_batch([]) == []
    # the object still works
    _check(_run_device(bird, frames[:2], ids[:2]), NF, frames[:2], ids[:2], "after the argument errors")


# ---------------------------------------------------------------- host form and group size
def test_host_form_equals_device_form(bird):
    frames, ids = bc.FIVE, [fr[2] for fr in bc.FIVE]
    dev = _run_device(bird, frames, ids)
    host = _run_host(bird, frames, ids)
    for f in range(5):
        assert dev[f][0].tobytes() == host[f][0].tobytes() and dev[f][1].tobytes() == host[f][1].tobytes(), f
    _check(host, NF, frames, ids, "host form")


@pytest.mark.parametrize("group", [1, 2, 64])
def test_group_size_does_not_change_results(orbgpu_mod, group):
    frames, ids = bc.FIVE, [fr[2] for fr in bc.FIVE]
    b = orbgpu_mod.BirdORB(NF)
    try:
        assert b.batch_group(group) == group and b.batch_group() == group
        _check(_run_device(b, frames, ids), NF, frames, ids, f"group {group}")
    finally:
        b.close()


# ---------------------------------------------------------------- the single calls: one frame of the same body
def _views_equal(b, cands, what):
    """debug_candidates(l) against the oracle's candidates of every level (test_bird_pyramid_and_candidates)."""
    for l in range(8):
        co, cg = cands[l], b.debug_candidates(l)
        assert len(cg) == len(co), f"{what}: level {l}: {len(cg)} vs {len(co)}"
        for f in ("x", "y", "octave", "class_id"):
            assert np.array_equal(cg[f], co[f]), (what, l, f)
        assert cg["response"].tobytes() == co["response"].tobytes(), f"{what}: Harris level {l}"


def _detect(b, nf, fr, mask_idx, what):
    kg = b.detect(bc.frame(*fr), bc.footprint_mask(fr[0], fr[1], mask_idx))
    ko = bc.detect_oracle(nf, fr, mask_idx)[0]
    assert len(kg) == len(ko), (what, len(kg), len(ko))
    assert kg.tobytes() == ko.tobytes(), (what, "detect")


def test_single_extract_second_download(orbgpu_mod):
    """A single extract whose frame has more candidates (55,495) than the 16,384 prefix of a fresh object, and
    keypoints culled after cornerSubPix; again with the grown prefix (one download); then a frame that fits."""
    scene, noise = (640, 480, 12, "scene"), (640, 480, 3, "noise")
    b = orbgpu_mod.BirdORB(2000)
    try:
        bc.assert_frame(b.extract(bc.frame(*noise)), 2000, noise, None, "noise, second download")
        bc.assert_frame(b.extract(bc.frame(*noise)), 2000, noise, None, "noise, one download")
        bc.assert_frame(b.extract(bc.frame(*scene), bc.mask(640, 480, 12).copy()), 2000, scene, 12, "scene")
    finally:
        b.close()
    assert bc.detected(2000, noise, None) - len(bc.expected(2000, noise, None)[0]) == 2


def test_single_calls_after_batch(orbgpu_mod):
    """After a batch of five the candidate buffer holds five slots: the single calls' prefix stays within one."""
    ids = [fr[2] for fr in bc.FIVE]
    noise = bc.FIVE[4]
    b = orbgpu_mod.BirdORB(NF)
    try:
        _check(_run_device(b, bc.FIVE, ids), NF, bc.FIVE, ids, "B=5")
        bc.assert_frame(b.extract(bc.frame(*noise), bc.mask(320, 240, 8).copy()), NF, noise, 8, "extract after B=5")
        _detect(b, NF, noise, 8, "detect after B=5")
        _detect(b, NF, noise, None, "detect after B=5, no mask")
    finally:
        b.close()


def test_debug_views(orbgpu_mod):
    """orb_bird_debug_candidates describes the last single detect or extract and nothing after a batch call."""
    from orbgpu import KP_DTYPE
    from orbgpu._lib import lib
    a, c = bc.FIVE[0], bc.FIVE[3]
    b = orbgpu_mod.BirdORB(NF)
    try:
        _detect(b, NF, a, a[2], "detect")
        _views_equal(b, bc.detect_oracle(NF, a, a[2])[1], "after detect")
        _check(_run_host(b, [a, c], [a[2], c[2]]), NF, [a, c], [a[2], c[2]], "B=2")
        out = np.zeros(1 << 16, KP_DTYPE)
        assert lib().orb_bird_debug_candidates(b.h, 0, out.ctypes.data_as(ctypes.c_void_p), len(out)) == ERR_ARG
        bc.assert_frame(b.extract(bc.frame(*c), bc.mask(320, 240, c[2]).copy()), NF, c, c[2], "extract")
        _views_equal(b, bc.detect_oracle(NF, c, c[2])[1], "after extract")
    finally:
        b.close()


def _raw_single(orbgpu_mod, bird, fr, mask_idx, cap, detect, poison=0xCD):
    """orb_bird_extract_device, or orb_bird_detect with the footprint mask, on poisoned outputs ->
    (status, n, kps, desc)."""
    import torch
    from orbgpu import KP_DTYPE
    from orbgpu._lib import lib
    w, h = fr[:2]
    kps = np.frombuffer(bytes([poison]) * (max(cap, 1) * KP_DTYPE.itemsize), KP_DTYPE).copy()
    desc = np.full((max(cap, 1), 32), poison, np.uint8)
    n = ctypes.c_int(-77)
    pk, pd = kps.ctypes.data_as(ctypes.c_void_p), desc.ctypes.data_as(ctypes.c_void_p)
    if detect:
        img, m = bc.frame(*fr), bc.footprint_mask(w, h, mask_idx)
        st = lib().orb_bird_detect(bird.h, img.ctypes.data_as(ctypes.c_void_p), w, h, w,
                                   m.ctypes.data_as(ctypes.c_void_p), w, pk, cap, ctypes.byref(n))
    else:
        di = torch.from_numpy(bc.frame(*fr).copy()).cuda()
        dm = torch.from_numpy(bc.mask(w, h, mask_idx).copy()).cuda()
        torch.cuda.synchronize()
        st = lib().orb_bird_extract_device(bird.h, ctypes.c_void_p(di.data_ptr()), w, h, w, ctypes.c_void_p(dm.data_ptr()),
                                           w, pk, cap, ctypes.byref(n), pd)
    return st, n.value, kps, desc


@pytest.mark.parametrize("detect", [False, True])
def test_capacity_single_calls(orbgpu_mod, bird, detect):
    fr, mi = bc.FIVE[0], bc.FIVE[0][2]
    ko, do = bc.expected(NF, fr, mi)
    if detect:
        ko = bc.detect_oracle(NF, fr, mi)[0]
    want = len(ko)
    assert want > 1
    st, n, kps, desc = _raw_single(orbgpu_mod, bird, fr, mi, want - 1, detect)
    assert st == ERR_CAPACITY and n == want
    assert _poisoned(kps) and _poisoned(desc)
    # with room for exactly the count the call succeeds; with two slots more, those keep their poison
    st, n, kps, desc = _raw_single(orbgpu_mod, bird, fr, mi, want, detect)
    assert st == 0 and n == want
    st2, n2, kps2, desc2 = _raw_single(orbgpu_mod, bird, fr, mi, want + 2, detect)
    assert st2 == 0 and n2 == want
    for k, d in ((kps, desc), (kps2, desc2)):
        assert k[:want].tobytes() == ko.tobytes()
        assert _poisoned(k[want:])
        if detect:
            assert _poisoned(d)
        else:
            assert d[:want].tobytes() == do.tobytes() and _poisoned(d[want:])


@pytest.mark.parametrize("batch_first", [True, False])
def test_single_call_equals_batch_of_one(orbgpu_mod, batch_first):
    """One frame through orb_bird_extract_batch_device and through orb_bird_extract_device on one object, in both
    orders: either call leaves the object's buffers fit for the other."""
    import torch
    fr, mi = bc.FIVE[3], bc.FIVE[3][2]
    di = torch.from_numpy(bc.frame(*fr).copy()).cuda()
    dm = torch.from_numpy(bc.mask(320, 240, mi).copy()).cuda()
    torch.cuda.synchronize()
    b = orbgpu_mod.BirdORB(NF)
    try:
        def single():
            k, d = b.extract_device(di.data_ptr(), 320, 240, dm.data_ptr())
            return k.copy(), d.copy()

        def batch():
            return b.extract_batch_device(di.data_ptr(), 1, 320, 240, d_masks=dm.data_ptr())[0]

        runs = [batch(), single(), batch()] if batch_first else [single(), batch(), single()]
        for i, r in enumerate(runs):
            bc.assert_frame(r, NF, fr, mi, f"run {i}")
            assert r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes(), i
    finally:
        b.close()
