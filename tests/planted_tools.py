"""What the planted-decision case files of the matchers share (tests/bow_cases.py, tests/triangulation_cases.py):
the two-sided builder of descriptors and FeatureVectors, and the rotation-histogram pair lists.  Pure numpy.
Also batch_levels, the pyramid levels of a batched extraction from a device buffer the test lays out
(tests/test_gpu_resize_rows.py, tests/test_gpu_pyramid_small.py)."""
import collections

import numpy as np

HISTO_LENGTH = 30

# rotation cases: the census items, the histogram's sizes by bin, ComputeThreeMaxima's answer, the culled matches
Rot = collections.namedtuple("Rot", "items sizes ind culled")


def sizes(d):
    return tuple(d.get(i, 0) for i in range(HISTO_LENGTH))


# (angle1, angle2) of one accepted pair each.  900 / 30 = 30.0: bin 30 -> 0; 15 * (1/30.f) == 0.5f exactly: round -> 1
ROT_BIN0 = [(0.0, 0.0), (100.0, 100.0), (7.0, 3.0), (900.0, 0.0)]
ROT_BIN1 = [(15.0, 0.0), (30.0, 0.0), (60.0, 25.0)]
# bins 0 and 1 tie at 10: bin 0 stays first (s > max1 is strict); bins 5 and 12 tie at 1: bin 5 is third, bin 12
# (10 - 20 + 360 = 350 -> 11.67 -> 12) is culled; max3 = 1 against 0.1f * 10 = 1.0: not below, kept
ROT_TIED = ROT_BIN0 + [(0.0, 0.0)] * 6 + ROT_BIN1 + [(30.0, 0.0)] * 7 + [(150.0, 0.0), (10.0, 20.0)]
ROT_TIED_EXPECTED = Rot(("rot_negative_wrap", "rot_bin_30_to_0", "rot_round_half", "maxima_first_second_tied",
                         "maxima_third_tied_first_wins", "maxima_third_at_cutoff_kept"),
                        sizes({0: 10, 1: 10, 5: 1, 12: 1}), (0, 1, 5), 1)


def batch_levels(orbgpu_mod, frames, scale, nlevels, variant, stride, base_off=0, runs=1):
    """Pyramid levels 1.. of every frame after each of `runs` batched extractions (the graph's capture, then replays)
    from a device buffer with row stride `stride` that starts `base_off` bytes into its allocation: [run][frame][l - 1]."""
    from orbgpu._lib import check, lib
    n, h, w = frames.shape
    e = orbgpu_mod.BatchExtractor(500, w, h, n, scale_factor=scale, nlevels=nlevels, variant=variant)
    padded = np.full((n, h, stride), 0xA5, np.uint8)   # the pad bytes are never read: any value must do
    padded[:, :, :w] = frames
    host = np.full(base_off + padded.nbytes, 0xA5, np.uint8)
    host[base_off:] = padded.reshape(-1)
    d = e._alloc(host.nbytes)
    try:
        check(lib().orb_memcpy_h2d(e.h, d, host.ctypes.data, host.nbytes), "h2d")
        out = []
        for _ in range(runs):
            check(lib().orb_extract_batch_device(e.h, d + base_off, n, w, h, stride * h, stride, e.d_kps, e.d_desc,
                                                 e.d_counts, e.kp_cap), "orb_extract_batch_device")
            e.sync()
            out.append([[e.debug_level_image(l, f) for l in range(1, nlevels)] for f in range(n)])
        return out
    finally:
        lib().orb_device_free(e.h, d)
        e.close()


class Builder:
    def __init__(self, name, seed, nnratio):
        self.name, self.nnratio = name, nnratio
        self.rng = np.random.default_rng(seed)
        self.d = ([], [])
        self.ang = ([], [])
        self.mp = ([], [])
        self.fv = ({}, {})
        self.plants = []
        self.fillers = []          # side-2 indices of random descriptors

    def rand(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    @staticmethod
    def flip(q, *ranges):
        m = np.zeros(256, np.uint8)
        for r in ranges:
            m[list(r)] ^= 1
        return q ^ np.packbits(m)

    def add(self, side, node, desc, mp=1, angle=0.0, pos=None):
        s = side - 1
        self.d[s].append(desc)
        self.ang[s].append(np.float32(angle))
        self.mp[s].append(mp)
        lst = self.fv[s].setdefault(node, [])
        lst.insert(len(lst) if pos is None else pos, len(self.d[s]) - 1)
        return len(self.d[s]) - 1

    def list_again(self, side, node, idx):
        self.fv[side - 1].setdefault(node, []).append(idx)

    def fill(self, node, n):
        for _ in range(n):
            self.fillers.append(self.add(2, node, self.rand()))

    def plant(self, item, idx1, kf_f, kf_kf="same"):
        self.plants.append(self.Plant(item, idx1, kf_f, kf_f if kf_kf == "same" else kf_kf))

    def simple(self, item, node, dists, kf_f, kf_kf="same"):
        """One query in its own node with candidates at the given distances (disjoint flip ranges)."""
        q = self.rand()
        i1 = self.add(1, node, q)
        out, at = [], 0
        for d in dists:
            out.append(self.add(2, node, self.flip(q, range(at, at + d))))
            at += d if at + 2 * d <= 256 else 0      # keep distinct descriptors while there is room
        fix = lambda e: e if e is None else (e[0], e[1], e[2], -1 if e[3] is None else out[e[3]])
        self.plant(item, i1, fix(kf_f), fix(kf_kf) if kf_kf != "same" else "same")
        return i1, out
