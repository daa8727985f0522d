"""What the pyramid tests of the one- and two-frame launches share (tests/test_pyramid_chain_host.py, the CPU model
and the oracle-only checks of the planted frames; tests/test_gpu_pyramid_small.py, the GPU parity): the sizes, the
planted frames and the device-buffer layouts.  Pure numpy."""
import numpy as np

GENERIC = 2   # VARIANT_RESIZE_GENERIC == ORACLE_RESIZE_GENERIC (tests/test_abi_cpu.py)

# (W, H, scale, nlevels).  What each holds is asserted from the model's output in tests/test_pyramid_chain_host.py.
EIGHT = [
    (331, 227, 1.2, 8),   # near the smallest frame 8 levels allow (level 7: 92 x 63); two segments on the host plan,
                          # the small plan chains levels 4..7 from level 3; level widths 133 (1 mod 4), 111 (3 mod 4)
    (333, 229, 1.2, 8),   # levels 3 and 4 (193, 161 wide) end in a one-pixel column of 32 x 16 tiles
]
OTHER = [
    (269, 210, 1.05, 6),
    (384, 241, 1.5, 4),   # level 1 is 256 x 161: a one-row last row of 64 x 32 tiles; KP = 3
    (700, 420, 1.9, 3),   # KP = 0; level 2 (194 wide) ends in a 2-pixel column of 64 x 32 tiles; still the packed form
    (400, 300, 2.2, 2),   # k_resize per level; the chain's byte form on the host path
    # found with the model, for what none of the above reaches
    (290, 193, 1.5, 3),   # level 1 is 193 x 129: one-pixel last column and one-row last row of 64 x 32 tiles
    (327, 219, 1.5, 4),   # level 3 is 97 x 65: the same of 32 x 16 tiles
    (260, 200, 2.1, 2),   # k_resize_tiled<32> with resize_tile's byte form (one 124-pixel tile column fits the LDS tile)
    (270, 200, 2.3, 2),   # k_resize_tiled<16, KP 0>: 32 output rows span more than 72 source rows, 16 do not
    (190, 200, 2.3, 2),   # k_resize_tiled<16, KP 2>
]
REFUSED = (820, 820, 1.9, 5)   # build_chain returns no plan for the host path (levels 1..4 from the frame at 1.9)
UNTILED = [(400, 300, 2.2, 2)]  # a level that k_resize takes: build_flow refuses the per-level dataflow launch
# The dataflow launch (ORBGPU_FLOW=1) gives each of 16 waves a FAST carve (fast_wave_bytes) and takes a geometry only
# when 16 of them fit a CU's LDS; near the smallest frame the top levels are one tall cell (331 x 227: level 5 is one
# 59-row cell) and the launch is refused.  Taller frames of the same level widths take it: the flow cases' 8-level sizes.
FLOW_EIGHT = [(331, 363, 1.2, 8), (333, 365, 1.2, 8)]
# the sizes of OTHER whose FAST carve fits (model: 16 * fast_wave_bytes <= 160 KiB - 64); 384 x 241, 270 x 200 and
# 190 x 200 do not
FLOW_OTHER = [(269, 210, 1.05, 6), (700, 420, 1.9, 3), (400, 300, 2.2, 2), (290, 193, 1.5, 3), (327, 219, 1.5, 4),
              (260, 200, 2.1, 2)]
# four chain jobs share the dataflow launch's LDS: a segment above (160 KiB - 64) / 4 - 256 bytes leaves the chain form out
CHAIN_TOO_LARGE = [(700, 420, 1.9, 3)]
SIZES = EIGHT + FLOW_EIGHT + OTHER + [REFUSED]

CONTENTS = ["noise", "all255", "zeros", "vstripes", "hstripes", "checker", "lastcolrow"]


def frame(w, h, content, seed=7):
    y, x = np.mgrid[0:h, 0:w]
    if content == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if content == "all255":        # the largest horizontal sum, 255 * 2048, at every pixel
        return np.full((h, w), 255, np.uint8)
    if content == "zeros":
        return np.zeros((h, w), np.uint8)
    if content == "vstripes":      # period 1: columns 0, 255, 0, ...
        return ((x & 1) * 255).astype(np.uint8)
    if content == "hstripes":
        return ((y & 1) * 255).astype(np.uint8)
    if content == "checker":       # 2 x 2 squares
        return ((((x >> 1) ^ (y >> 1)) & 1) * 255).astype(np.uint8)
    if content == "lastcolrow":    # the last column and the last row alone: the clamped coefficients, the base load's tail
        f = np.zeros((h, w), np.uint8)
        f[:, -1] = 255
        f[-1, :] = 255
        return f
    raise ValueError(content)


def frames(w, h, content, n):
    """n frames of one content: frame 1 is other noise, or the inverse of the planted frame."""
    f0 = frame(w, h, content)
    return np.stack([f0, frame(w, h, content, 8) if content == "noise" else 255 - f0][:n])


LAYOUTS = ["s64", "s4", "packed", "off1"]


def layout(w, name):
    """(row stride, base offset) of a device buffer: a 64-byte multiple; a multiple of 4 but not of 16; the packed
    width (odd at the 8-level sizes: the second frame's base is odd); a 64-byte multiple from an odd base."""
    r4 = (w + 3) & ~3
    return {"s64": ((w + 63) & ~63, 0), "s4": (r4 if r4 % 16 else r4 + 4, 0), "packed": (w, 0),
            "off1": ((w + 63) & ~63, 1)}[name]
