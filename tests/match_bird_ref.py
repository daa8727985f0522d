"""Test-side restatement of the reference's SearchByMatchBird (src/ORBmatcher.cc), loop by loop, in float32 / int
arithmetic, over plain arrays:

  search_kf_f     SearchByMatchBird(KeyFrame* pKF, Frame& F, vector<MapPointBird*>&, r)          :2000-2114
  birdview_match  BirdviewMatch(const Frame& F1, const Frame& F2, vector<int>&, windowSize)      :1790-1899
  search_frame    SearchByMatchBird(Frame& CurrentFrame, const Frame& LastFrame, windowSize)     :1901-1921

MapPointBird* is replaced by the index k of the keyframe's (the last frame's) birdview keypoint that owns it.  A
Frame is a dict: desc (n, 32) uint8 = mDescriptorsBird, kps (KP_DTYPE) = mvKeysBird, bounds = (0, birdviewCols, 0,
birdviewRows).  The pieces the oracle already pins are the oracle's, as in projection_ref: features_in_area
(GetFeaturesInAreaBirdview is Frame::GetFeaturesInArea over the birdview grid, Frame.cc:891-945), rot_bin,
three_maxima.

search_kf_f returns (match, nmatches, counters): match[t] = the k whose map point train t holds last, -1 = never
assigned, -2 = reset to NULL by the rotation cull; counters count the branches taken (COUNTERS).
"""
import numpy as np

TH_HIGH = 100          # ORBmatcher.cc:37
TH_LOW = 50            # :38
HISTO_LENGTH = 30      # :39
INT_MAX = 2 ** 31 - 1
f32 = np.float32

COUNTERS = ("steals", "le_skips", "seconds_at_256", "different_level_accepts", "culled_entries",
            "culled_entries_on_reset_or_reowned", "exhausted_queries")

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def descriptor_distance(a, b):   # :1647-1663
    return int(_POP[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum())


def _exhausted(cands, table, k):
    """The k smallest-distance candidates (first in candidate order on ties) are all inadmissible, more remain."""
    if len(cands) <= k:
        return False
    top = sorted((d, pos, idx) for pos, (idx, d) in enumerate(cands))[:k]
    return all(table[idx] <= d for d, _, idx in top)


def search_kf_f(oracle, kf, frame, r, nnratio, check_ori, max_dist=TH_HIGH, topk=8):
    """:2000-2114.  kf: index (the k with vpMapPointsBirdKF[k] != NULL, ascending as the loop visits them), x, y
    (pKF->mvKeysBird[k].pt), angle, desc (pMPBird->GetDescriptor()).  topk only feeds the exhausted_queries counter."""
    nt = len(frame["kps"])
    match = np.full(nt, -1, np.int64)                                                # :2004
    matched_distance = [INT_MAX] * nt                                                # :2005
    octave = frame["kps"]["octave"]
    c = {k: 0 for k in COUNTERS}
    nmatches = 0                                                                     # :2007
    rot_hist = [[] for _ in range(HISTO_LENGTH)]                                     # :2009 (train, k) per entry
    for i in range(len(kf["index"])):                                                # :2014 (NULL ones left out)
        k = int(kf["index"][i])
        x, y = f32(kf["x"][i]), f32(kf["y"][i])
        ind = oracle.features_in_area(frame["kps"], *frame["bounds"], float(x), float(y), float(f32(r)))   # :2023
        if len(ind) == 0:                                                            # :2025
            continue
        best_dist, best_level, best_dist2, best_level2, best_idx = INT_MAX, -1, INT_MAX, -1, -1   # :2030-2034
        cands = []
        for idx in ind.tolist():                                                     # :2037
            dist = descriptor_distance(kf["desc"][i], frame["desc"][idx])            # :2047
            cands.append((idx, dist))
            if matched_distance[idx] <= dist:                                        # :2051
                c["le_skips"] += 1
                continue
            if dist < best_dist:                                                     # :2054-2066
                best_dist2, best_dist = best_dist, dist
                best_level2, best_level = best_level, int(octave[idx])
                best_idx = idx
            elif dist < best_dist2:
                best_level2, best_dist2 = int(octave[idx]), dist
        if _exhausted(cands, matched_distance, topk):
            c["exhausted_queries"] += 1
        if best_dist <= max_dist:                                                    # :2070
            ratio_ok = bool(f32(best_dist) < f32(best_dist2) * f32(nnratio))         # (float)bestDist2*mfNNratio
            if best_dist2 == 256:
                c["seconds_at_256"] += 1
            if best_level != best_level2 or ratio_ok:                                # :2072
                if not ratio_ok and best_level2 != -1:
                    c["different_level_accepts"] += 1
                if match[best_idx] >= 0:
                    c["steals"] += 1
                match[best_idx] = k                                                  # :2074
                matched_distance[best_idx] = best_dist                               # :2075
                if check_ori:                                                        # :2077-2087
                    b = oracle.rot_bin(float(f32(kf["angle"][i])), float(frame["kps"]["angle"][best_idx]))
                    rot_hist[b].append((best_idx, k))
                nmatches += 1                                                        # :2088
    if check_ori:                                                                    # :2093-2111
        keep = oracle.three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for t, k in rot_hist[b]:
                if match[t] != k:     # already reset by an earlier entry, or owned by a later query by now
                    c["culled_entries_on_reset_or_reowned"] += 1
                match[t] = -2                                                        # :2107
                nmatches -= 1                                                        # :2108
                c["culled_entries"] += 1
    return match, nmatches, c


def birdview_match(oracle, f1, f2, window, nnratio, check_ori):
    """:1790-1899.  Returns (vnMatches12, nmatches)."""
    n1, n2 = len(f1["kps"]), len(f2["kps"])
    matches12 = np.full(n1, -1, np.int64)                                            # :1791
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    matched_distance = [INT_MAX] * n2                                                # :1798
    matches21 = [-1] * n2                                                            # :1799
    nmatches = 0
    for i1 in range(n1):                                                             # :1801
        kp1 = f1["kps"][i1]
        level1 = int(kp1["octave"])
        ind = oracle.features_in_area(f2["kps"], *f2["bounds"], float(kp1["x"]), float(kp1["y"]),
                                      float(f32(int(window))), level1, level1)       # :1808
        if len(ind) == 0:
            continue
        best_dist, best_dist2, best_idx2 = INT_MAX, INT_MAX, -1                      # :1815-1817
        for i2 in ind.tolist():
            dist = descriptor_distance(f1["desc"][i1], f2["desc"][i2])
            if matched_distance[i2] <= dist:                                         # :1827
                continue
            if dist < best_dist:
                best_dist2, best_dist, best_idx2 = best_dist, dist, i2
            elif dist < best_dist2:
                best_dist2 = dist
        if best_dist <= TH_LOW:                                                      # :1842
            if f32(best_dist) < f32(best_dist2) * f32(nnratio):                      # :1844
                if matches21[best_idx2] >= 0:                                        # :1846-1850
                    matches12[matches21[best_idx2]] = -1
                    nmatches -= 1
                matches12[i1] = best_idx2
                matches21[best_idx2] = i1
                matched_distance[best_idx2] = best_dist
                nmatches += 1
                if check_ori:                                                        # :1856-1866
                    rot_hist[oracle.rot_bin(float(kp1["angle"]), float(f2["kps"]["angle"][best_idx2]))].append(i1)
    if check_ori:                                                                    # :1872-1896
        keep = oracle.three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in rot_hist[b]:
                if matches12[idx1] >= 0:
                    matches21[matches12[idx1]] = -1
                    matches12[idx1] = -1
                    nmatches -= 1
    return matches12, nmatches


def carry_over(matches12, has_mp_last, n_cur):
    """:1907-1918: (match_cur, nmatches, matched points without a map point)."""
    match_cur = np.full(n_cur, -1, np.int64)
    nmatches = without = 0
    for k in range(len(matches12)):                                                  # :1907
        idx2 = int(matches12[k])
        if idx2 < 0:
            continue
        if has_mp_last is not None and has_mp_last[k]:                               # :1912-1913
            match_cur[idx2] = k                                                      # :1915
            nmatches += 1
        else:
            without += 1
    return match_cur, nmatches, without


def search_frame(oracle, cur, last, window, nnratio, check_ori, has_mp_last):
    """:1901-1921.  Returns (match_cur, nmatches, counters): counters = BirdviewMatch's own return value and the
    matched points that carry no map point."""
    matches12, n12 = birdview_match(oracle, last, cur, window, nnratio, check_ori)   # :1905
    match_cur, nmatches, without = carry_over(matches12, has_mp_last, len(cur["kps"]))
    return match_cur, nmatches, dict(birdview_matches=n12, matched_without_map_point=without)
