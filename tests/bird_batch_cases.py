"""Frames, masks and oracle results shared by the batched birdview tests (tests/test_gpu_bird_batch*.py).

A frame is (w, h, idx, kind); its mask is synth_bird_mask(w, h, mask_idx).  expected() is the oracle's
Frame.cc:320-342 for one frame and mask alone, computed once per (frame, mask, nfeatures)."""
import functools

import numpy as np

# the five distinct 320x240 frames of the batch-size tests: the flat one in the middle, the noise one last
FIVE = [(320, 240, 7, "scene"), (320, 240, 11, "scene"), (320, 240, 10, "flat"), (320, 240, 13, "scene"),
        (320, 240, 8, "noise")]


@functools.lru_cache(maxsize=None)
def frame(w, h, idx, kind="scene"):
    from orbgpu.synth import synth_frame
    f = synth_frame(w, h, idx, kind)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def mask(w, h, idx):
    from orbgpu.synth import synth_bird_mask
    m = synth_bird_mask(w, h, idx)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(nf, fr, mask_idx):
    """(keypoints, descriptors) of oracle.OracleCvORB(nf).extract(frame, mask); mask_idx None: no mask."""
    import oracle
    w, h = fr[0], fr[1]
    k, d = oracle.OracleCvORB(nf).extract(frame(*fr), None if mask_idx is None else mask(w, h, mask_idx).copy())
    return k, d


def footprint_mask(w, h, mask_idx):
    """The mask detect sees inside extract: the footprint zeroed (None: no mask)."""
    if mask_idx is None:
        return None
    import orbgpu
    return orbgpu.bird_footprint_mask(mask(w, h, mask_idx))


@functools.lru_cache(maxsize=None)
def detect_oracle(nf, fr, mask_idx):
    """(keypoints of the oracle's detect with the footprint mask, its candidates per level)."""
    import oracle
    o = oracle.OracleCvORB(nf)
    k = o.detect(frame(*fr), footprint_mask(fr[0], fr[1], mask_idx))
    return k, [o.candidates(l) for l in range(8)]


def detected(nf, fr, mask_idx):
    """Keypoints the oracle's detect keeps before cornerSubPix and the border cull of compute."""
    return len(detect_oracle(nf, fr, mask_idx)[0])


def assert_frame(got, nf, fr, mask_idx, what):
    """got = (keypoints, descriptors) of one frame of a batch: byte equality with the oracle, named by `what`."""
    ko, do = expected(nf, fr, mask_idx)
    kg, dg = got
    assert len(kg) == len(ko), (what, len(kg), len(ko))
    assert kg.tobytes() == ko.tobytes(), (what, "keypoints")
    assert np.asarray(dg).tobytes() == do.tobytes(), (what, "descriptors")
