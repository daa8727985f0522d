"""GPU parity of k_resize_rows, the pyramid resize of the batch path's per-level launches: every level of every
frame byte-identical to the oracle's (OracleExtractor.level).

The batch is 3 frames, the smallest that takes the per-level plan (kChainMaxFrames = 2 frames and fewer take the
few-launch pyramid).  Frames are uploaded with a row stride of their own: a 64-byte multiple lets level 1 (read
from the frames) take the kernel too, an odd one sends level 1 down the unaligned staging path of k_resize_tiled
while the levels above still take it.  Level sizes are round(size / scale^l) (ComputePyramid); the cases put level 1
 * one below, at and one above the tile width 256, which are also 3, 0 and 1 mod 4 (the last lane's clamped group);
 * at heights that leave a one-row last tile (161 = 5 * 32 + 1) and a one-row last strip (169 = 5 * 32 + 8 + 1);
and run scale 1.2, 1.05 (nearly every source row shared by two output rows), 1.5, 1.9 (the widest byte window the
kernel takes) and 2.2 (source rows skipped: the geometry leaves the level to the other kernels), and the generic
vertical pass (VARIANT_RESIZE_GENERIC).  The host-side geometry and index arithmetic have a CPU model,
tests/test_resize_rows_host.py."""
import numpy as np
import pytest

from gpu_tools import batch_levels

pytestmark = pytest.mark.gpu

B = 3
RESIZE = 2   # VARIANT_RESIZE_GENERIC == ORACLE_RESIZE_GENERIC (tests/test_abi_cpu.py)


def _levels(orbgpu_mod, frames, scale, nlevels, variant, stride):
    """Pyramid levels 1.. of every frame after one batched extraction from a device buffer with row stride `stride`."""
    return batch_levels(orbgpu_mod, frames, scale, nlevels, variant, stride)[0]


@pytest.mark.parametrize("w,h,scale,nlevels,variant,stride", [
    (306, 193, 1.2, 4, 0, 320),        # level 1: 255 x 161
    (307, 203, 1.2, 4, 0, 320),        # 256 x 169
    (308, 193, 1.2, 4, 0, 320),        # 257 x 161
    (307, 193, 1.2, 4, RESIZE, 320),   # the generic vertical pass
    (308, 203, 1.2, 4, RESIZE, 309),   # and with level 1 through the unaligned staging path
    (307, 203, 1.2, 4, 0, 307),        # packed frames of odd width, as BatchExtractor.upload lays them out
    (269, 210, 1.05, 6, 0, 320),       # 256 x 200, then 244, 232, 221, 211 wide
    (384, 241, 1.5, 3, 0, 384),        # 256 x 161
    (520, 300, 1.9, 2, 0, 576),        # 274 x 158
    (520, 300, 1.9, 2, RESIZE, 576),
    (400, 300, 2.2, 2, 0, 448),        # 182 x 136: not this kernel's (k_resize_tiled's byte path / k_resize)
])
def test_batch_levels_match_the_oracle(orbgpu_mod, oracle_mod, w, h, scale, nlevels, variant, stride):
    from orbgpu.synth import synth_frame
    frames = np.stack([synth_frame(w, h, 11 + f, "noise" if f == 1 else "scene") for f in range(B)])
    got = _levels(orbgpu_mod, frames, scale, nlevels, variant, stride)
    o = oracle_mod.OracleExtractor(500, scale, nlevels, flags=variant)
    for f in range(B):
        o(frames[f])
        for l in range(1, nlevels):
            ref = o.level(l)
            assert got[f][l - 1].shape == ref.shape, (f, l, got[f][l - 1].shape, ref.shape)
            bad = np.argwhere(got[f][l - 1] != ref)
            assert len(bad) == 0, (f, l, len(bad), bad[:4].tolist())
