"""A hand-written DBoW2 vocabulary file and planted features that put the vocabulary loader's re-layout and
k_vocab_transform's descent at their edges.  Pure numpy and struct; tests/test_vocab_cases.py checks on the CPU that
tests/vocab_ref.py and the oracle agree and that every census item is realised; tests/test_gpu_vocab_cases.py loads
the same files into the product and runs the same features.

The tree (k = 3, L = 3), records in depth-first order, node id = record number:

    1 A (root's child)            2 A1 (of 1)     3 A1a  4 A1b (weight 0: a stopped word)  5 A1c   (leaves, depth 3)
                                  6 A2 (of 1)     7 A2a                                            (one child, depth 2)
    8 B  (a leaf at depth 1)
    9 Ca (of 10: its parent's record comes later)   10 C (of root)   11 Cb (of 10, descriptor identical to Ca's)
    12 Cc (of 10; the last record, which the loader's end-of-file quirk stores again as node 13, one more child of C
       and one more word)

So children are not contiguous by id (root: 1, 8, 10; C: 9, 11, 12, 13), child counts are 1, 2, 3 and 4, and leaves sit
at depths 1, 2 and 3.  A child's descriptor is its parent's with a fixed range of bits flipped; a feature is a
leaf's descriptor with up to five of bits 200..255 flipped, far inside that leaf's margin (siblings differ by 20 bits or
more), or a descriptor placed at exactly equal distance from two siblings.  Built once, never modified."""
import functools
import struct

import numpy as np

from planted_tools import Builder

K, L = 3, 3
flip = Builder.flip

ITEMS = (
    "leaf_at_depth_1", "leaf_at_depth_L", "node_with_1_child", "node_with_2_children", "node_with_k_children",
    "records_depth_first", "parent_id_above_child", "children_not_contiguous", "identical_sibling_descriptors",
    "equal_distance_first_child_wins", "nearest_is_last_record", "eof_duplicate_record", "stopped_word",
    "n_1", "n_255", "n_256", "n_257", "levelsup_0", "levelsup_L_minus_1", "levelsup_L", "levelsup_L_plus_2",
    "nid_uninitialised_reads_0", "all_words_stopped", "two_features_share_a_word", "every_scoring_weighting_pair",
)

LEVELSUP = {"levelsup_0": 0, "levelsup_L_minus_1": L - 1, "levelsup_L": L, "levelsup_L_plus_2": L + 2}
COUNTS = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def tree():
    """[(parent, descriptor, weight, is_leaf)] in record order, and the descriptors by name."""
    rng = np.random.default_rng(51)
    A, B, C = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(3))
    A1, A2 = flip(A, range(0, 40)), flip(A, range(40, 80))
    d = dict(A=A, B=B, C=C, A1=A1, A2=A2, A1a=flip(A1, range(100, 120)), A1b=flip(A1, range(120, 140)),
             A1c=flip(A1, range(140, 160)), A2a=flip(A2, range(100, 110)), Ca=flip(C, range(0, 20)),
             Cc=flip(C, range(20, 40)))
    d["Cb"] = d["Ca"].copy()
    rec = [(0, "A", 0.0, 0), (1, "A1", 0.0, 0), (2, "A1a", 1.5, 1), (2, "A1b", 0.0, 1), (2, "A1c", 2.25, 1),
           (1, "A2", 0.0, 0), (6, "A2a", 0.75, 1), (0, "B", 1.25, 1), (10, "Ca", 0.5, 1), (0, "C", 0.0, 0),
           (10, "Cb", 3.0, 1), (10, "Cc", 2.0, 1)]
    return tuple((p, d[n], w, leaf) for p, n, w, leaf in rec), d, tuple(n for _, n, _, _ in rec)


def write(path, scoring=0, weighting=0):
    rec, _, _ = tree()
    with open(path, "wb") as f:
        f.write(struct.pack("<IIiiii", len(rec) + 1, 41, K, L, scoring, weighting))
        for parent, desc, w, leaf in rec:
            f.write(struct.pack("<i", parent) + desc.tobytes() + struct.pack("<f", w) + bytes([leaf]))


# name -> (descriptor, expected node id of the leaf, expected word id, expected weight).  Word ids count the leaf
# records in file order: A1a 0, A1b 1, A1c 2, A2a 3, B 4, Ca 5, Cb 6, Cc 7 (and the duplicate 8).
@functools.lru_cache(maxsize=None)
def base_features():
    _, d, _ = tree()
    out = {
        "A1a": (d["A1a"], 3, 0, 1.5), "A1b": (d["A1b"], 4, 1, 0.0), "A1c": (d["A1c"], 5, 2, 2.25),
        "A2a": (d["A2a"], 7, 3, 0.75), "B": (d["B"], 8, 4, 1.25),
        "Ca": (d["Ca"], 9, 5, 0.5),          # Cb (node 11) is identical: the first of the two wins
        "Cc": (d["Cc"], 12, 7, 2.0),         # node 13 is its duplicate: the first wins, word 7 not 8
        # 10 bits towards A1a and 10 towards A1b from A1: 20 from either, 40 from A1c: the first child wins
        "A1a_A1b_tie": (flip(d["A1"], range(100, 110), range(120, 130)), 3, 0, 1.5),
    }
    return out


def features(n, seed=0, names=None):
    """n features cycling through the base features (or `names`), each with up to five of bits 200..255 flipped.
    Returns (descriptors, names)."""
    rng = np.random.default_rng(1000 + seed)
    base = base_features()
    names = list(base) if names is None else list(names)
    out, who = [], []
    for i in range(n):
        nm = names[i % len(names)]
        bits = 200 + rng.choice(56, int(rng.integers(0, 6)), replace=False)
        out.append(flip(base[nm][0], bits.tolist()))
        who.append(nm)
    a = np.stack(out)
    a.setflags(write=False)
    return a, who


ALL_STOPPED = ("A1b",)                      # every feature lands on the stopped word
SHARED = ("A1a", "A1a", "Cc", "B")          # two features share word 0
PAIRS = tuple((s, w) for s in range(6) for w in range(4))
