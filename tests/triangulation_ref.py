"""Plain Python restatement of ORBmatcher::SearchForTriangulation (ORBmatcher.cc:657-823) and CheckDistEpipolarLine
(:140-157), written from the reference source.  Float arithmetic is numpy float32, one rounding per operation (the
unfused form); the final comparison is in double as in the source (3.84 is a double literal).  Returns the pairs and a
trace: per visited feature of KF1 its candidates with the reason each was dropped or kept."""
import numpy as np

from bow_ref import HISTO_LENGTH, TH_LOW, common_nodes, descriptor_distance, rot_bin, three_maxima

f32 = np.float32
HAS_MP, MONO, NONE, MATCHED = "has a map point", "not stereo", "no candidate kept", "matched"


def check_dist_epipolar_line(kp1, kp2, F12, sigma2):
    """Returns (ok, den, dsqr)."""
    x1, y1, x2, y2 = f32(kp1["x"]), f32(kp1["y"]), f32(kp2["x"]), f32(kp2["y"])
    F = np.asarray(F12, f32).reshape(3, 3)
    a = f32(f32(f32(x1 * F[0, 0]) + f32(y1 * F[1, 0])) + F[2, 0])
    b = f32(f32(f32(x1 * F[0, 1]) + f32(y1 * F[1, 1])) + F[2, 1])
    c = f32(f32(f32(x1 * F[0, 2]) + f32(y1 * F[1, 2])) + F[2, 2])
    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
    den = f32(f32(a * a) + f32(b * b))
    if den == 0:
        return False, den, None
    dsqr = f32(f32(num * num) / den)
    return float(dsqr) < 3.84 * float(f32(sigma2[kp2["octave"]])), den, dsqr


def search_for_triangulation(check_ori, only_stereo, desc1, kps1, mp1, ur1, fv1, desc2, kps2, mp2, ur2, fv2, F12, ex,
                             ey, scale2, sigma2_2):
    ex, ey = f32(ex), f32(ey)
    matched2 = [False] * len(desc2)              # never set by the source (:677): a train can be matched twice
    matches12 = [-1] * len(desc1)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    visits = []
    nodes, _ = common_nodes(fv1, fv2)
    for node in nodes:
        for idx1 in fv1[node]:
            rec = dict(node=node, idx1=idx1, outcome=None, best=-1, best_dist=None, cands=[], bin=None)
            visits.append(rec)
            if mp1[idx1]:
                rec["outcome"] = HAS_MP
                continue
            stereo1 = ur1[idx1] >= 0
            if only_stereo and not stereo1:
                rec["outcome"] = MONO
                continue
            kp1 = kps1[idx1]
            best_dist, best_idx2 = TH_LOW, -1
            for idx2 in fv2[node]:
                def drop(why, **kw):
                    rec["cands"].append(dict(idx2=idx2, why=why, **kw))
                if matched2[idx2] or mp2[idx2]:
                    drop("mp")
                    continue
                stereo2 = ur2[idx2] >= 0
                if only_stereo and not stereo2:
                    drop("stereo")
                    continue
                dist = descriptor_distance(desc1[idx1], desc2[idx2])
                if dist > TH_LOW or dist > best_dist:
                    drop("dist", dist=dist, best_dist=best_dist)
                    continue
                kp2 = kps2[idx2]
                if not stereo1 and not stereo2:
                    distex = f32(ex - f32(kp2["x"]))
                    distey = f32(ey - f32(kp2["y"]))
                    e2 = f32(f32(distex * distex) + f32(distey * distey))
                    lim = f32(f32(100) * f32(scale2[kp2["octave"]]))
                    if e2 < lim:
                        drop("epipole", dist=dist, e2=e2, lim=lim)
                        continue
                    gate = dict(e2=e2, lim=lim)
                else:
                    gate = dict(e2=None, lim=None)
                ok, den, dsqr = check_dist_epipolar_line(kp1, kp2, F12, sigma2_2)
                if ok:
                    best_idx2, best_dist = idx2, dist
                    drop("kept", dist=dist, den=den, dsqr=dsqr, **gate)
                else:
                    drop("den" if den == 0 else "line", dist=dist, den=den, dsqr=dsqr, **gate)
            rec.update(best=best_idx2, best_dist=best_dist, outcome=MATCHED if best_idx2 >= 0 else NONE)
            if best_idx2 >= 0:
                matches12[idx1] = best_idx2
                nmatches += 1
                if check_ori:
                    b, _ = rot_bin(kp1["angle"], kps2[best_idx2]["angle"])
                    rec["bin"] = b
                    rot_hist[b].append(idx1)
    sizes = [len(h) for h in rot_hist]
    ind, culled = None, 0
    if check_ori:
        ind = three_maxima(sizes)
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for j in rot_hist[i]:
                matches12[j] = -1
                nmatches -= 1
                culled += 1
    pairs = np.array([(i, m) for i, m in enumerate(matches12) if m >= 0], np.int32).reshape(-1, 2)
    assert len(pairs) == nmatches
    return pairs, dict(visits=visits, sizes=sizes, ind=ind, culled=culled)
