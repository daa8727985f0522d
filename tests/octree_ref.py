"""DistributeOctTree and ExtractorNode::DivideNode (ORBextractor.cc:477-763) restated in plain Python, with a trace.

The node list is a Python list used the way the reference uses its std::list (children go in with insert(0, ...),
a divided node is deleted where it stands); the phase-2 vector of (size, node) pairs is sorted with the pinned tie
policy of the oracle (equal sizes: the earlier-created node counts as the smaller pointer) or its reverse
(ORB_VARIANT_TIE_REVERSE / ORACLE_TIE_REVERSE_SEQ).  Nothing here is shared with k_octree: no path codes, no count
tables, no counting sort, no packed words.

distribute(keys, minX, maxX, minY, maxY, N, reverse_tie) takes the keys in vToDistributeKeys order as (x, y, response)
relative to the min border and returns (result, trace): the retained keys in list order, and what every round did."""
import math

import numpy as np

f32 = np.float32


class Node:
    __slots__ = ("x0", "x1", "y0", "y1", "keys", "nomore", "seq", "depth", "parent")

    def __init__(self, x0, x1, y0, y1, depth):
        self.x0, self.x1, self.y0, self.y1 = x0, x1, y0, y1    # UL.x, UR.x, UL.y, BR.y
        self.keys = []                                          # (x, y, response, index in vToDistributeKeys)
        self.nomore = False
        self.seq = -1
        self.parent = -1
        self.depth = depth

    def divide(self):                                           # :477-535
        half_x = math.ceil((self.x1 - self.x0) / 2)
        half_y = math.ceil((self.y1 - self.y0) / 2)
        xm, ym = self.x0 + half_x, self.y0 + half_y
        d = self.depth + 1
        n1 = Node(self.x0, xm, self.y0, ym, d)
        n2 = Node(xm, self.x1, self.y0, ym, d)
        n3 = Node(self.x0, xm, ym, self.y1, d)
        n4 = Node(xm, self.x1, ym, self.y1, d)
        for k in self.keys:
            if k[0] < xm:
                (n1 if k[1] < ym else n3).keys.append(k)
            elif k[1] < ym:
                n2.keys.append(k)
            else:
                n4.keys.append(k)
        for n in (n1, n2, n3, n4):
            n.parent = self.seq
            if len(n.keys) == 1:
                n.nomore = True
        return n1, n2, n3, n4


def _index(lst, node):
    for i, n in enumerate(lst):
        if n is node:
            return i
    raise ValueError("node not in the list")


def distribute(keys, minX, maxX, minY, maxY, N, reverse_tie=False):
    n_ini = int(round(float(f32(maxX - minX) / f32(maxY - minY))))        # :543 (no input here sits on .5)
    hx = f32(maxX - minX) / f32(n_ini)
    trace = {"nIni": n_ini, "hX": float(hx), "rounds": [], "roots": [], "divisions": []}
    roots = []
    seq = 0
    for i in range(n_ini):
        r = Node(int(hx * f32(i)), int(hx * f32(i + 1)), 0, maxY - minY, 0)
        r.seq = seq
        seq += 1
        roots.append(r)
    for i, (x, y, resp) in enumerate(keys):
        roots[int(f32(x) / hx)].keys.append((int(x), int(y), int(resp), i))
    lst = []
    for r in roots:                                                       # :572-585
        trace["roots"].append((r.x0, r.x1, len(r.keys)))
        if len(r.keys) == 1:
            r.nomore = True
        if r.keys:
            lst.append(r)

    def push(c, vec):
        nonlocal seq
        if not c.keys:
            return 0
        c.seq = seq
        seq += 1
        lst.insert(0, c)
        if len(c.keys) > 1:
            vec.append((len(c.keys), c))
        return 1

    def divided(node, children):
        trace["divisions"].append({"depth": node.depth, "rect": (node.x0, node.x1, node.y0, node.y1),
                                   "xm": children[0].x1, "ym": children[0].y1, "keys": [k[:2] for k in node.keys],
                                   "nonempty": sum(1 for c in children if c.keys)})

    finish = False
    while not finish:                                                     # :594
        prev = len(lst)
        vec = []
        i = 0
        while i < len(lst):
            nd = lst[i]
            if nd.nomore:
                i += 1
                continue
            ch = nd.divide()
            divided(nd, ch)
            for c in ch:
                i += push(c, vec)
            del lst[i]
        n_expand = len(vec)
        trace["rounds"].append({"phase": 1, "before": prev, "after": len(lst), "nToExpand": n_expand,
                                "multi_pos": [p for p, n in enumerate(lst) if len(n.keys) > 1]})
        if len(lst) >= N or len(lst) == prev:                             # :669
            finish = True
        elif len(lst) + n_expand * 3 > N:                                 # :673
            while not finish:
                prev = len(lst)
                where = {id(n): p for p, n in enumerate(lst)}
                pv = sorted(vec, key=lambda p: (p[0], -p[1].seq if reverse_tie else p[1].seq))   # :684
                vec = []
                sizes = [p[0] for p in pv]
                cut = None
                for j in range(len(pv) - 1, -1, -1):
                    nd = pv[j][1]
                    ch = nd.divide()
                    divided(nd, ch)
                    for c in ch:
                        push(c, vec)
                    del lst[_index(lst, nd)]
                    if len(lst) >= N:                                     # :730
                        cut = j
                        break
                trace["rounds"].append({"phase": 2, "before": prev, "after": len(lst), "nToExpand": len(vec),
                                        "sorted": [(p[0], p[1].seq, p[1].depth, p[1].parent, where[id(p[1])])
                                                   for p in pv],
                                        "cut": cut, "ties": sorted({s for s in sizes if sizes.count(s) > 1})})
                if len(lst) >= N or len(lst) == prev:
                    finish = True
    result, final = [], []
    for pos, nd in enumerate(lst):                                        # :741-762
        best = nd.keys[0]
        for k in nd.keys[1:]:
            if k[2] > best[2]:
                best = k
        result.append(best[:3])
        final.append({"rect": (nd.x0, nd.x1, nd.y0, nd.y1), "count": len(nd.keys), "best": best, "pos": pos,
                      "depth": nd.depth, "tied_max": sum(1 for k in nd.keys if k[2] == best[2]) > 1,
                      "best_at": [k[3] for k in nd.keys].index(best[3]),
                      "has253": any(k[2] == 253 for k in nd.keys),
                      "raster_other": any(k[2] == best[2] and (k[1], k[0]) < (best[1], best[0]) for k in nd.keys)})
    trace["final"] = final
    return result, trace
