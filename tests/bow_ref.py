"""Plain Python restatements of ORBmatcher::SearchByBoW(KeyFrame*, Frame&) (ORBmatcher.cc:159-288) and
SearchByBoW(KeyFrame*, KeyFrame*) (:522-655) with the rotation histogram and ComputeThreeMaxima (:1601-1642), written
from the reference source, one statement per statement.  Each returns the matches and a trace: one record per keyframe
feature in visit order, and the histogram's state.  tests/triangulation_ref.py and tests/window_ref.py share the
helpers."""
import numpy as np

f32 = np.float32
TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30
NO_MP, DIST, RATIO, ACCEPTED = "no map point", "bestDist1 above TH_LOW", "ratio test", "accepted"


def descriptor_distance(a, b):
    return int(np.unpackbits(a ^ b).sum())


def c_round(x):
    """round(): halves away from zero."""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def rot_bin(a1, a2):
    """:238-243.  Returns (bin, rot*factor) ; float arithmetic."""
    factor = f32(1.0) / f32(HISTO_LENGTH)
    rot = f32(a1) - f32(a2)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    v = f32(rot * factor)
    b = c_round(v)
    if b == HISTO_LENGTH:
        b = 0
    assert 0 <= b < HISTO_LENGTH
    return b, v


def three_maxima(sizes):
    """ComputeThreeMaxima (:1601-1642) on the bins' sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(f32(0.1) * f32(max1)):
        ind2 = ind3 = -1
    elif f32(max3) < f32(f32(0.1) * f32(max1)):
        ind3 = -1
    return ind1, ind2, ind3


def common_nodes(fv1, fv2):
    """The merge of two FeatureVectors (std::map: ascending node id) with lower_bound (:180-264).  Yields the common
    node ids; skips[0] / skips[1] count the lower_bound jumps on either side."""
    k1, k2 = sorted(fv1), sorted(fv2)
    i = j = 0
    out, skips = [], [0, 0]
    while i < len(k1) and j < len(k2):
        if k1[i] == k2[j]:
            out.append(k1[i])
            i += 1
            j += 1
        elif k1[i] < k2[j]:
            i = next((p for p in range(i, len(k1)) if k1[p] >= k2[j]), len(k1))      # lower_bound
            skips[0] += 1
        else:
            j = next((p for p in range(j, len(k2)) if k2[p] >= k1[i]), len(k2))
            skips[1] += 1
    return out, skips


def _cull(rot_hist, reset):
    ind = three_maxima([len(h) for h in rot_hist])
    n = 0
    for i in range(HISTO_LENGTH):
        if i in ind:
            continue
        for j in rot_hist[i]:
            reset(j)
            n += 1
    return ind, n


def search_by_bow(form, nnratio, check_ori, desc1, angle1, mp1, fv1, desc2, angle2, mp2, fv2):
    """form "kf_f": 1 = the keyframe, 2 = the Frame (mp2 unused); returns (nmatches, match_f[n2], trace).
    form "kf_kf": returns (nmatches, match12[n1], trace).  mp: non-zero = a MapPoint that is not bad."""
    kf_f = form == "kf_f"
    nnratio = f32(nnratio)
    matches = [-1] * (len(desc2) if kf_f else len(desc1))
    matched2 = [False] * len(desc2)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    visits = []
    nodes, skips = common_nodes(fv1, fv2)
    for node in nodes:
        for idx1 in fv1[node]:
            rec = dict(node=node, idx1=idx1, outcome=NO_MP, d1=None, d2=None, best=-1, bin=None, rotf=None, seen=0)
            visits.append(rec)
            if not mp1[idx1]:
                continue
            best1, best_idx, best2 = 256, -1, 256
            for idx2 in fv2[node]:
                if kf_f:
                    if matches[idx2] >= 0:
                        continue
                elif matched2[idx2] or not mp2[idx2]:
                    continue
                rec["seen"] += 1
                dist = descriptor_distance(desc1[idx1], desc2[idx2])
                if dist < best1:
                    best2, best1, best_idx = best1, dist, idx2
                elif dist < best2:
                    best2 = dist
            rec.update(d1=best1, d2=best2, best=best_idx)
            if not (best1 <= TH_LOW if kf_f else best1 < TH_LOW):
                rec["outcome"] = DIST
                continue
            if not f32(best1) < f32(nnratio * f32(best2)):
                rec["outcome"] = RATIO
                continue
            rec["outcome"] = ACCEPTED
            if kf_f:
                matches[best_idx] = idx1
            else:
                matches[idx1] = best_idx
                matched2[best_idx] = True
            if check_ori:
                b, v = rot_bin(angle1[idx1], angle2[best_idx])
                rec.update(bin=b, rotf=v)
                rot_hist[b].append(best_idx if kf_f else idx1)
            nmatches += 1
    ind, culled = (None, 0)
    sizes = [len(h) for h in rot_hist]
    if check_ori:
        def reset(j):
            matches[j] = -1
        ind, culled = _cull(rot_hist, reset)
        nmatches -= culled
    trace = dict(visits=visits, skips=skips, nodes=nodes, sizes=sizes, ind=ind, culled=culled)
    return nmatches, np.array(matches, np.int32), trace
