"""Plain Python restatement, written from the reference source, of DBoW2's TemplatedVocabulary for ORB descriptors:
loadFromBinaryFile (TemplatedVocabulary.h:1466-1510, its end-of-file quirk included: the loop runs once more after the
last record and stores that record again as one more node), the per-feature descent (:1230-1271) and transform's
BowVector / FeatureVector assembly (:1139-1206, BowVector.cpp:34-84)."""
import math
import struct

import numpy as np

TF_IDF, TF, IDF, BINARY = range(4)
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
SIZE_NODE = 4 + 32 + 4 + 1


class Node:
    def __init__(self):
        self.parent, self.children, self.descriptor, self.weight, self.word_id = 0, [], None, 0.0, None


class Vocabulary:
    def __init__(self, path):
        with open(path, "rb") as f:
            data = f.read()
        nb_nodes, size_node, self.k, self.L, self.scoring, self.weighting = struct.unpack_from("<IIiiii", data, 0)
        assert size_node == SIZE_NODE
        self.nodes = [Node() for _ in range(nb_nodes + 1)]
        self.words = []
        pos, nid, buf, eof = 24, 1, None, False
        while not eof:                                  # while (!f.eof())
            chunk = data[pos:pos + size_node]
            pos += size_node
            if len(chunk) == size_node:
                buf = chunk
            else:
                eof = True                              # the read fails, buf keeps the last record
            n = self.nodes[nid]
            n.parent = struct.unpack_from("<i", buf, 0)[0]
            self.nodes[n.parent].children.append(nid)
            n.descriptor = np.frombuffer(buf, np.uint8, 32, 4).copy()
            n.weight = struct.unpack_from("<f", buf, 36)[0]
            if buf[40]:
                n.word_id = len(self.words)
                self.words.append(nid)
            nid += 1

    def transform_one(self, feature, levelsup):
        """(word_id, weight, nid, path): nid is None where the source leaves it uninitialised."""
        nid_level = self.L - levelsup
        nid = 0 if nid_level <= 0 else None
        final_id, level, path = 0, 0, []
        while True:
            level += 1
            nodes = self.nodes[final_id].children
            final_id = nodes[0]
            best_d = int(np.unpackbits(feature ^ self.nodes[final_id].descriptor).sum())
            tied = False
            for i in nodes[1:]:
                d = int(np.unpackbits(feature ^ self.nodes[i].descriptor).sum())
                if d < best_d:
                    best_d, final_id, tied = d, i, False
                elif d == best_d:
                    tied = True
            path.append((final_id, best_d, tied, len(nodes)))
            if level == nid_level:
                nid = final_id
            if not self.nodes[final_id].children:
                break
        return self.nodes[final_id].word_id, self.nodes[final_id].weight, nid, path

    def transform(self, features, levelsup):
        """(BowVector as {word: value}, FeatureVector as {node: [feature indices]})."""
        must, norm = {L1_NORM: (True, 1), L2_NORM: (True, 2), CHI_SQUARE: (True, 1), KL: (True, 1),
                      BHATTACHARYYA: (True, 1), DOT_PRODUCT: (False, 1)}[self.scoring]
        v, fv = {}, {}
        for i, f in enumerate(features):
            wid, w, nid, _ = self.transform_one(f, levelsup)
            if w > 0:
                if self.weighting in (TF, TF_IDF):
                    v[wid] = v.get(wid, 0.0) + w          # addWeight
                else:
                    v.setdefault(wid, w)                  # addIfNotExist
                fv.setdefault(nid, []).append(i)
        if self.weighting in (TF, TF_IDF) and v and not must:
            nd = float(len(v))
            for k in v:
                v[k] /= nd
        if must:
            s = 0.0
            for k in sorted(v):
                s += abs(v[k]) if norm == 1 else v[k] * v[k]
            if norm == 2:
                s = math.sqrt(s)
            if s > 0.0:
                for k in v:
                    v[k] /= s
        return dict(sorted(v.items())), dict(sorted(fv.items(), key=lambda kv: (kv[0] is None, kv[0])))
