"""Test-side restatement of the reference's keyframe searches (src/ORBmatcher.cc), in float32 / int arithmetic over
plain arrays:

  fuse_search          the inner search of Fuse(KeyFrame*, const vector<MapPoint*>&, th)            :892-949  (chi2=True)
                       and of Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, th, ...)       :1051-1079 (chi2=False)
  search_by_sim3       SearchBySim3's two inner searches :1191-1219 / :1271-1299 and the agreement loop :1308-1323
  search_kf_scw        SearchByProjection(KeyFrame*, cv::Mat Scw, vpPoints, vpMatched, th)          :290-403
  search_f_kf          SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)            :1472-1599

MapPoint* is replaced by the index of the projected point.  A keyframe / frame is a dict: desc (n, 32) uint8, kps
(KP_DTYPE, mvKeysUn), bounds (mnMinX, mnMaxX, mnMinY, mnMaxY), uright (mvuRight) or None, inv_sigma2
(mvInvLevelSigma2).  Points are dicts of arrays: u, v, level (nPredictedLevel), radius (th * mvScaleFactors[level]),
desc, and ur / angle / index where the search reads them.  The points the reference skips before its search (isBad,
already found, negative depth, !IsInImage, the distance and viewing-angle tests) are assumed filtered, as the
product's entry points assume.  KeyFrame::GetFeaturesInArea(u, v, r) is the oracle's features_in_area(..., -1, -1)
(KeyFrame.cc:586-625 is Frame::GetFeaturesInArea without levels); descriptor_distance, rot_bin and three_maxima are
the oracle's too.

fuse_search returns the first minimum per point (best_idx, best_dist; -1 / -1 where no candidate passes) before any
threshold: Fuse(KF, vpMapPoints) starts its running minimum at 256 and the other bodies at INT_MAX, which differ only
for a distance of 256, above every threshold the callers apply.  Counters count the branches taken (COUNTERS)."""
from fractions import Fraction

import numpy as np

TH_LOW, TH_HIGH = 50, 100     # ORBmatcher.cc:37-38
HISTO_LENGTH = 30             # :39
f32 = np.float32

COUNTERS = ("level_skips", "chi2_stereo_rejections", "chi2_mono_rejections", "ties_first_kept", "taken_skips",
            "rotation_culls", "sim3_disagreements")


def counters():
    return {k: 0 for k in COUNTERS}


def round_f32(x):
    """The float32 nearest to the rational x (ties to even), computed on integers: no rounding through float64."""
    x = Fraction(x)
    if x == 0:
        return f32(0.0)
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()     # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                    # 2^e <= a < 2^(e+1)
    e = max(e, -126)                                              # subnormals share the smallest normal's quantum
    quantum = Fraction(2) ** (e - 23)
    n = a / quantum
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2 == 1):
        k += 1
    out = float(sign * k * quantum)                               # k < 2^25: exact in float64 and in float32
    assert abs(out) < 2.0 ** 128
    return f32(out)


def fmaf(a, b, c):
    """float32 fma: a * b + c rounded once."""
    return round_f32(Fraction(float(f32(a))) * Fraction(float(f32(b))) + Fraction(float(f32(c))))


def fuse_e2(u, v, ur, kpx, kpy, kpr):
    """e2 of ORBmatcher.cc:914-938 in the reference build's contracted forms (tools/fuse_flags_probe.cpp): stereo
    (kpr >= 0) fmaf(er, er, fmaf(ex, ex, ey * ey)), mono fmaf(ex, ex, ey * ey).  Returns (e2, stereo)."""
    ex, ey = f32(f32(u) - f32(kpx)), f32(f32(v) - f32(kpy))
    e2 = fmaf(ex, ex, f32(ey * ey))
    if f32(kpr) >= 0:                                                                # :914
        er = f32(f32(ur) - f32(kpr))
        return fmaf(er, er, e2), True
    return e2, False


def fuse_gate_skips(u, v, ur, kpx, kpy, kpr, inv_sigma2):
    """(skipped, stereo): `if(e2*pKF->mvInvLevelSigma2[kpLevel]>7.8) continue;` (:925) / `>5.99` (:936): a float
    product compared with a double constant."""
    e2, stereo = fuse_e2(u, v, ur, kpx, kpy, kpr)
    return float(f32(e2 * f32(inv_sigma2))) > (7.8 if stereo else 5.99), stereo


def _area(oracle, kf, u, v, r):
    return oracle.features_in_area(kf["kps"], *kf["bounds"], float(u), float(v), float(r), -1, -1).tolist()


def best_in_area(oracle, kf, u, v, ur, level, radius, desc, chi2, c, level_above=0):
    """One point's inner search: (best_idx, best_dist)."""
    kps = kf["kps"]
    uright = None if kf.get("uright") is None else np.asarray(kf["uright"], f32)
    best_dist, best_idx = None, -1
    for idx in _area(oracle, kf, u, v, radius):                                       # :903 / :1062 / :1201 / :1281
        kp_level = int(kps["octave"][idx])
        if kp_level < level - 1 or kp_level > level + level_above:                    # :911 / :1067 / :1207 / :1287
            c["level_skips"] += 1
            continue
        if chi2:                                                                      # :914-938
            kpr = f32(-1) if uright is None else uright[idx]
            skipped, stereo = fuse_gate_skips(u, v, ur, kps["x"][idx], kps["y"][idx], kpr, kf["inv_sigma2"][kp_level])
            if skipped:
                c["chi2_stereo_rejections" if stereo else "chi2_mono_rejections"] += 1
                continue
        dist = oracle.descriptor_distance(desc, kf["desc"][idx])                      # :942 / :1072 / :1212 / :1292
        if best_dist is None or dist < best_dist:                                     # :944-948
            best_dist, best_idx = dist, idx
        elif dist == best_dist:
            c["ties_first_kept"] += 1
    return (best_idx, best_dist) if best_idx >= 0 else (-1, -1)


def fuse_search(oracle, kf, pts, chi2):
    """Per point (best_idx, best_dist) as two int arrays, and the counters."""
    n = len(pts["u"])
    bi, bd, c = np.full(n, -1, np.int64), np.full(n, -1, np.int64), counters()
    for i in range(n):
        ur = pts["ur"][i] if chi2 else 0.0
        bi[i], bd[i] = best_in_area(oracle, kf, pts["u"][i], pts["v"][i], ur, int(pts["level"][i]), pts["radius"][i],
                                    pts["desc"][i], chi2, c)
    return bi, bd, c


def fuse_one(oracle, kf, pts, i, desc, chi2):
    """Point i of pts with another descriptor (a point whose descriptor changed during the replay)."""
    ur = pts["ur"][i] if chi2 else 0.0
    return best_in_area(oracle, kf, pts["u"][i], pts["v"][i], ur, int(pts["level"][i]), pts["radius"][i], desc, chi2,
                        counters())


def search_by_sim3(oracle, kf1, kf2, pts1in2, pts2in1):
    """:1102-1326 from the two lists of projected points (index = the point's feature in its own keyframe)."""
    c = counters()
    n1, n2 = len(kf1["kps"]), len(kf2["kps"])
    vn1, vn2 = np.full(n1, -1, np.int64), np.full(n2, -1, np.int64)                  # :1144-1145
    for pts, kf, vn in ((pts1in2, kf2, vn1), (pts2in1, kf1, vn2)):
        for k in range(len(pts["u"])):
            bi, bd = best_in_area(oracle, kf, pts["u"][k], pts["v"][k], 0.0, int(pts["level"][k]), pts["radius"][k],
                                  pts["desc"][k], False, c)
            if bi >= 0 and bd <= TH_HIGH:                                             # :1221 / :1301
                vn[int(pts["index"][k])] = bi
    out = np.full(n1, -1, np.int64)
    nfound = 0
    for i1 in range(n1):                                                              # :1310-1323
        idx2 = vn1[i1]
        if idx2 >= 0:
            if vn2[idx2] == i1:
                out[i1] = idx2
                nfound += 1
            else:
                c["sim3_disagreements"] += 1
    return nfound, out, c


def _sequential(oracle, pts, frame, taken, max_dist, level_above, check_ori):
    nt = len(frame["kps"])
    match = np.full(nt, -1, np.int64)
    taken = np.asarray(taken, bool).copy()
    octave = frame["kps"]["octave"]
    c = counters()
    nmatches = 0
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    for i in range(len(pts["u"])):
        level = int(pts["level"][i])
        if level_above:                                                               # :1528: levels in the grid query
            ind = oracle.features_in_area(frame["kps"], *frame["bounds"], float(pts["u"][i]), float(pts["v"][i]),
                                          float(pts["radius"][i]), level - 1, level + level_above).tolist()
        else:                                                                         # :362
            ind = _area(oracle, frame, pts["u"][i], pts["v"][i], pts["radius"][i])
        best_dist, best_idx = 256, -1                                                 # :370-371 / :1535-1536
        for idx in ind:
            if taken[idx]:                                                            # :375 / :1541
                c["taken_skips"] += 1
                continue
            if not level_above and (octave[idx] < level - 1 or octave[idx] > level):  # :380
                c["level_skips"] += 1
                continue
            dist = oracle.descriptor_distance(pts["desc"][i], frame["desc"][idx])     # :385 / :1546
            if dist < best_dist:
                best_dist, best_idx = dist, idx
            elif dist == best_dist:
                c["ties_first_kept"] += 1
        if best_dist <= max_dist:                                                     # :394 / :1555
            match[best_idx] = i                                                       # :396 / :1557
            taken[best_idx] = True
            nmatches += 1
            if check_ori:                                                             # :1560-1570
                rot_hist[oracle.rot_bin(float(pts["angle"][i]), float(frame["kps"]["angle"][best_idx]))].append(best_idx)
    if check_ori:                                                                     # :1577-1596
        keep = oracle.three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for t in rot_hist[b]:
                    match[t] = -2
                    nmatches -= 1
                    c["rotation_culls"] += 1
    return match, nmatches, c


def search_kf_scw(oracle, pts, kf, matched):
    """:290-403.  matched[idx] = vpMatched[idx] != NULL.  Returns (match, nmatches, counters): match[idx] = the point
    the call assigned to feature idx, -1 where it assigned none."""
    return _sequential(oracle, pts, kf, matched, TH_LOW, 0, False)


def search_f_kf(oracle, pts, frame, has_mp, orb_dist, check_ori):
    """:1472-1599.  has_mp[i2] = CurrentFrame.mvpMapPoints[i2] != NULL; pts additionally angle (pKF->mvKeysUn[i]
    .angle).  match[i2] = -2 where the rotation cull reset the feature to NULL."""
    return _sequential(oracle, pts, frame, has_mp, int(orb_dist), 1, check_ori)
