"""Test-side restatement of the reference's three projection-gated searches (src/ORBmatcher.cc), loop by loop, in
float32 / int arithmetic, over plain arrays:

  search_cf_lf        SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)   :1328-1470
  search_f_mappoints  SearchByProjection(Frame& F, const vector<MapPoint*>&, th)                   :45-129
  search_bird         SearchByProjectionBird(Frame& F, const vector<MapPointBird*>&, r)            :1923-1998

MapPoint* is replaced by the index of the query (the projected map point); a Frame is a dict

  desc (n, 32) uint8, kps (KP_DTYPE: mvKeysUn / mvKeysBird), bounds (mnMinX, mnMaxX, mnMinY, mnMaxY),
  uright (n float32, mvuRight; -1 = none) or None, taken (n bool: mvpMapPoints[i] && Observations() > 0) or None.

The points the reference skips before its search (outliers, !mbTrackInView, isBad, invzc < 0, out of bounds) are
assumed filtered, as the product's entry point assumes.  The pieces the oracle already pins are the oracle's:
features_in_area (Frame::GetFeaturesInArea), descriptor_distance, rot_bin, three_maxima.

Each function returns (match, nmatches, counters): match[t] = index of the last query assigned to train t, -1 =
never assigned, -2 = reset to NULL by the rotation cull; counters count the branches taken (COUNTERS).
"""
import numpy as np

TH_HIGH = 100          # ORBmatcher.cc:37
HISTO_LENGTH = 30      # :39
f32 = np.float32

COUNTERS = ("stereo_rejections", "ratio_rejections_same_level", "accepted_different_level_despite_ratio",
            "taken_skips", "zero_observation_overwrites", "rotation_culls")


def _counters():
    return {k: 0 for k in COUNTERS}


def _taken0(frame):
    n = len(frame["kps"])
    return np.zeros(n, bool) if frame.get("taken") is None else np.asarray(frame["taken"], bool).copy()


def _uright(frame):
    n = len(frame["kps"])
    return np.full(n, -1, f32) if frame.get("uright") is None else np.asarray(frame["uright"], f32)


def radius_by_viewing_cos(view_cos):   # :131-137 (a float compared with the double 0.998)
    return f32(2.5) if float(f32(view_cos)) > 0.998 else f32(4.0)


def running_two_smallest(dists, levels):
    """The reference's running update (:76-115): (bestDist, bestLevel, bestIdx, bestDist2, bestLevel2)."""
    best, lvl, idx, best2, lvl2 = 256, -1, -1, 256, -1
    for i, (d, l) in enumerate(zip(dists, levels)):
        if d < best:
            best2, lvl2 = best, lvl
            best, lvl, idx = d, l, i
        elif d < best2:
            best2, lvl2 = d, l
    return best, lvl, idx, best2, lvl2


def sorted_two_smallest(dists, levels):
    """The same five values as the first two entries of the (dist, position) order among distances below 256."""
    order = sorted((d, i) for i, d in enumerate(dists) if d < 256)
    best, lvl, idx, best2, lvl2 = 256, -1, -1, 256, -1
    if order:
        best, idx = order[0]
        lvl = levels[idx]
    if len(order) > 1:
        best2 = order[1][0]
        lvl2 = levels[order[1][1]]
    return best, lvl, idx, best2, lvl2


def search_cf_lf(oracle, pts, cf, th, b_mono, check_ori, b_forward=False, b_backward=False):
    """:1328-1470.  pts: u, v, invzc (float32), octave (LastFrame.mvKeys[i].octave), angle (LastFrame.mvKeysUn[i]
    .angle), observed (pMP->Observations() > 0), desc.  cf additionally: scale_factors (mvScaleFactors), mbf."""
    nt = len(cf["kps"])
    match = np.full(nt, -1, np.int64)
    observed = _taken0(cf)            # CurrentFrame.mvpMapPoints[i2] && Observations() > 0
    uright = _uright(cf)
    c = _counters()
    nmatches = 0
    rot_hist = [[] for _ in range(HISTO_LENGTH)]                                     # :1333
    b_forward = bool(b_forward) and not b_mono                                       # :1348-1349
    b_backward = bool(b_backward) and not b_mono
    scale = np.asarray(cf["scale_factors"], f32)
    for i in range(len(pts["u"])):                                                   # :1351
        u, v, invzc = f32(pts["u"][i]), f32(pts["v"][i]), f32(pts["invzc"][i])
        oct_ = int(pts["octave"][i])                                                 # :1378
        radius = f32(th) * scale[oct_]                                               # :1381
        if b_forward:                                                                # :1385-1390
            lv = (oct_, -1)
        elif b_backward:
            lv = (0, oct_)
        else:
            lv = (oct_ - 1, oct_ + 1)
        ind = oracle.features_in_area(cf["kps"], *cf["bounds"], float(u), float(v), float(radius), *lv)
        if len(ind) == 0:                                                            # :1392
            continue
        best_dist, best_idx = 256, -1                                                # :1397-1398
        for i2 in ind.tolist():                                                      # :1400
            if observed[i2]:                                                         # :1403-1405
                c["taken_skips"] += 1
                continue
            if uright[i2] > 0:                                                       # :1407-1413
                ur = f32(u - f32(f32(cf["mbf"]) * invzc))
                er = abs(f32(ur - uright[i2]))
                if er > radius:
                    c["stereo_rejections"] += 1
                    continue
            dist = oracle.descriptor_distance(pts["desc"][i], cf["desc"][i2])        # :1417
            if dist < best_dist:                                                     # :1419-1423
                best_dist, best_idx = dist, i2
        if best_dist <= TH_HIGH:                                                     # :1426
            if match[best_idx] >= 0:
                c["zero_observation_overwrites"] += 1
            match[best_idx] = i                                                      # :1428
            observed[best_idx] = bool(pts["observed"][i])
            nmatches += 1
            if check_ori:                                                            # :1431-1441
                rot_hist[oracle.rot_bin(float(pts["angle"][i]), float(cf["kps"]["angle"][best_idx]))].append(best_idx)
    if check_ori:                                                                    # :1448-1467
        keep = oracle.three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for t in rot_hist[b]:
                    match[t] = -2
                    nmatches -= 1
                    c["rotation_culls"] += 1
    return match, nmatches, c


def _ratio_search(oracle, frame, nnratio, windows, qdesc, stereo):
    """The shared body of :51-126 and :1929-1995: windows[i] = (x, y, r, minLevel, maxLevel, projXR or None)."""
    nt = len(frame["kps"])
    match = np.full(nt, -1, np.int64)
    observed = _taken0(frame)
    uright = _uright(frame)
    octave = frame["kps"]["octave"]
    c = _counters()
    nmatches = 0
    for i, (x, y, r, lmin, lmax, xr) in enumerate(windows):
        ind = oracle.features_in_area(frame["kps"], *frame["bounds"], float(x), float(y), float(r), lmin, lmax)
        if len(ind) == 0:                                                            # :71 / :1947
            continue
        best_dist, best_level, best_dist2, best_level2, best_idx = 256, -1, 256, -1, -1   # :76-80 / :1952-1956
        for idx in ind.tolist():                                                     # :83 / :1959
            if observed[idx]:                                                        # :87-89 / :1963-1965
                c["taken_skips"] += 1
                continue
            if stereo and uright[idx] > 0:                                           # :91-96
                er = abs(f32(f32(xr) - uright[idx]))
                if er > f32(r):
                    c["stereo_rejections"] += 1
                    continue
            dist = oracle.descriptor_distance(qdesc[i], frame["desc"][idx])          # :100 / :1969
            if dist < best_dist:                                                     # :102-114 / :1971-1983
                best_dist2, best_dist = best_dist, dist
                best_level2, best_level = best_level, int(octave[idx])
                best_idx = idx
            elif dist < best_dist2:
                best_level2, best_dist2 = int(octave[idx]), dist
        if best_dist <= TH_HIGH:                                                     # :118 / :1987
            over = f32(best_dist) > f32(nnratio) * f32(best_dist2)
            if best_level == best_level2 and over:                                   # :120-121 / :1989-1990
                c["ratio_rejections_same_level"] += 1
                continue
            if over:
                c["accepted_different_level_despite_ratio"] += 1
            if match[best_idx] >= 0:
                c["zero_observation_overwrites"] += 1
            match[best_idx] = i                                                      # :123 / :1992
            observed[best_idx] = True   # (the map points of these two searches have observations)
            nmatches += 1
    return match, nmatches, c


def search_f_mappoints(oracle, pts, frame, th, nnratio):
    """:45-129.  pts: proj_x, proj_y, proj_xr (mTrackProjX / Y / XR), level (mnTrackScaleLevel), view_cos
    (mTrackViewCos), desc.  frame additionally: scale_factors."""
    scale = np.asarray(frame["scale_factors"], f32)
    b_factor = f32(th) != 1.0                                                        # :49
    windows = []
    for i in range(len(pts["level"])):
        lv = int(pts["level"][i])                                                    # :60
        r = radius_by_viewing_cos(pts["view_cos"][i])                                # :63
        if b_factor:                                                                 # :65-66
            r = f32(r * f32(th))
        rr = f32(r * scale[lv])                                                      # :69, :94
        windows.append((f32(pts["proj_x"][i]), f32(pts["proj_y"][i]), rr, lv - 1, lv, f32(pts["proj_xr"][i])))
    return _ratio_search(oracle, frame, nnratio, windows, pts["desc"], True)


def search_bird(oracle, pts, frame, r, nnratio):
    """:1923-1998.  pts: x, y (the birdview projection pt, :1940), desc.  frame: the birdview features
    (mvKeysBird, mDescriptorsBird, mvpMapPointsBird), bounds = (0, birdviewCols, 0, birdviewRows)."""
    windows = [(f32(pts["x"][i]), f32(pts["y"][i]), f32(r), -1, -1, None) for i in range(len(pts["x"]))]   # :1945
    return _ratio_search(oracle, frame, nnratio, windows, pts["desc"], False)
