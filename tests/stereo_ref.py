"""Test-side restatement of Frame::ComputeStereoMatches (src/Frame.cc:662-836), loop by loop, in float32 / int
arithmetic over plain arrays:

  levels_l / levels_r   mpORBextractorLeft / Right->mvImagePyramid as uint8 arrays (OracleExtractor.level(l))
  scale / inv_scale     mvScaleFactors / mvInvScaleFactors of the left extractor (Frame.cc:104-109)
  kps_*, desc_*         mvKeys / mvKeysRight (KP_DTYPE) and mDescriptors / mDescriptorsRight ((n, 32) uint8)

Returns (mvuRight, mvDepth, nmatched, trace).  nmatched counts the entries that survive the median cut.  trace holds
one entry per left keypoint (arrays of length N) plus the cut's scalars:

  ncand      len(vRowIndices[vL])                                  :707
  best_idx   bestIdxR, -1 while bestDist is still TH_HIGH          :718-745
  best_dist  bestDist of the descriptor search (100 = nothing below TH_HIGH)
  outcome    one of OUTCOMES
  bestinc    bestincR (0 where the window search did not run)      :763-788
  vdists     the 11 window distances (nan where the search did not run)
  sad        the int bestDist pushed into vDistIdx (-1 = not pushed)   :817
  median, th_dist   :823-824 (nan when vDistIdx is empty)

Where the reference indexes unchecked (vRowIndices[yi] for a band that leaves the image, vDistIdx[0] of an empty
vector) this restatement skips the row / returns no match; tests/stereo_cases.py keeps every band inside the image.
"""
import math

import numpy as np

f32 = np.float32
TH_HIGH, TH_LOW = 100, 50          # ORBmatcher.cc:37-38
W_HALF, L_RANGE = 5, 5             # :758 w, :765 L

NO_CANDIDATE = "no candidate"              # :709 / :715
DIST_HIGH = "dist >= 75"                   # :748 fails
WINDOW_OFF = "window off the image"        # :771
BEST_AT_L = "best at +-L"                  # :790
DELTA_RANGE = "deltaR out of [-1, 1]"      # :800 (unreachable for a minimum of non-negative distances)
DISPARITY_RANGE = "disparity out of range"  # :808 fails
CLAMPED = "clamped to 0.01"                # :810-814, and kept by the cut
ACCEPTED = "accepted"                      # kept by the cut
CUT = "cut"                                # :826-835
OUTCOMES = (NO_CANDIDATE, DIST_HIGH, WINDOW_OFF, BEST_AT_L, DELTA_RANGE, DISPARITY_RANGE, CLAMPED, ACCEPTED, CUT)


def c_round(x):
    """round() of a float: halves away from zero."""
    x = float(x)
    return f32(math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5))


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance (ORBmatcher.cc:1647-1663): the popcount of the XOR of 256 bits."""
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def compute_stereo_matches(levels_l, levels_r, scale, inv_scale, kps_l, desc_l, kps_r, desc_r, mb, mbf):
    N, Nr = len(kps_l), len(kps_r)
    scale = np.asarray(scale, f32)
    inv_scale = np.asarray(inv_scale, f32)
    uright = np.full(N, -1, f32)                                                     # :664-665
    depth = np.full(N, -1, f32)
    trace = dict(ncand=np.zeros(N, np.int64), best_idx=np.full(N, -1, np.int64), best_dist=np.full(N, TH_HIGH, np.int64),
                 outcome=[NO_CANDIDATE] * N, bestinc=np.zeros(N, np.int64), vdists=np.full((N, 2 * L_RANGE + 1), np.nan, f32),
                 sad=np.full(N, -1, np.int64), median=float("nan"), th_dist=float("nan"))
    th_orb_dist = (TH_HIGH + TH_LOW) // 2                                            # :667
    n_rows = levels_l[0].shape[0]                                                    # :669
    # :679-689: keypoint iR is pushed to rows minr..maxr, in iR order; row yi's list is therefore the ascending iR
    # with minr <= yi <= maxr (rows outside the image: see the module docstring)
    kr_x = np.asarray(kps_r["x"], f32)
    kr_oct = np.asarray(kps_r["octave"], np.int64)
    r = f32(2.0) * scale[kr_oct] if Nr else np.zeros(0, f32)
    maxr = np.ceil((np.asarray(kps_r["y"], f32) + r).astype(f32)).astype(np.int64)
    minr = np.floor((np.asarray(kps_r["y"], f32) - r).astype(f32)).astype(np.int64)
    min_z = f32(mb)                                                                  # :692-694
    min_d = f32(0)
    max_d = f32(f32(mbf) / min_z)
    v_dist_idx = []
    for iL in range(N):                                                              # :700
        level_l = int(kps_l["octave"][iL])
        vL, uL = f32(kps_l["y"][iL]), f32(kps_l["x"][iL])
        row = int(vL)                                                                # :707 (float index, truncated)
        cands = np.flatnonzero((minr <= row) & (row <= maxr)) if 0 <= row < n_rows else np.zeros(0, np.int64)
        trace["ncand"][iL] = len(cands)
        if len(cands) == 0:                                                          # :709
            continue
        min_u = f32(uL - max_d)                                                      # :712-713
        max_u = f32(uL - min_d)
        if max_u < 0:                                                                # :715
            continue
        best_dist, best_idx = TH_HIGH, 0                                             # :718-719
        for iR in cands.tolist():                                                    # :724
            if kr_oct[iR] < level_l - 1 or kr_oct[iR] > level_l + 1:                 # :729
                continue
            uR = kr_x[iR]
            if uR >= min_u and uR <= max_u:                                          # :734
                dist = descriptor_distance(desc_l[iL], desc_r[iR])
                if dist < best_dist:                                                 # :739
                    best_dist, best_idx = dist, iR
        trace["best_dist"][iL] = best_dist
        trace["best_idx"][iL] = best_idx if best_dist < TH_HIGH else -1
        if not best_dist < th_orb_dist:                                              # :748
            trace["outcome"][iL] = DIST_HIGH
            continue
        uR0 = kr_x[best_idx]                                                         # :751-755
        scale_factor = inv_scale[level_l]
        scaled_uL = c_round(f32(uL * scale_factor))
        scaled_vL = c_round(f32(vL * scale_factor))
        scaled_uR0 = c_round(f32(uR0 * scale_factor))
        w, L = W_HALF, L_RANGE
        PL, PR = levels_l[level_l], levels_r[level_l]
        y0, xl = int(scaled_vL), int(scaled_uL)
        assert y0 - w >= 0 and y0 + w < PL.shape[0] and xl - w >= 0 and xl + w < PL.shape[1], "left window off the level"
        IL = PL[y0 - w:y0 + w + 1, xl - w:xl + w + 1].astype(np.int64)               # :759-761 (exact in float)
        IL = IL - IL[w, w]
        iniu = f32(scaled_uR0 + f32(L) - f32(w))                                     # :769-772
        endu = f32(scaled_uR0 + f32(L) + f32(w) + f32(1))
        if iniu < 0 or endu >= PR.shape[1]:
            trace["outcome"][iL] = WINDOW_OFF
            continue
        best_dist2, bestinc = 2 ** 31 - 1, 0                                         # :763-764
        v_dists = np.zeros(2 * L + 1, f32)
        xr = int(scaled_uR0)
        assert xr - L - w >= 0, "right window off the level"
        for inc in range(-L, L + 1):                                                 # :774-788
            IR = PR[y0 - w:y0 + w + 1, xr + inc - w:xr + inc + w + 1].astype(np.int64)
            IR = IR - IR[w, w]
            dist = f32(np.abs(IL - IR).sum())                                        # cv::norm NORM_L1: an exact integer
            if dist < best_dist2:
                best_dist2, bestinc = int(dist), inc
            v_dists[L + inc] = dist
        trace["bestinc"][iL] = bestinc
        trace["vdists"][iL] = v_dists
        if bestinc == -L or bestinc == L:                                            # :790
            trace["outcome"][iL] = BEST_AT_L
            continue
        dist1, dist2, dist3 = v_dists[L + bestinc - 1], v_dists[L + bestinc], v_dists[L + bestinc + 1]   # :794-798
        with np.errstate(divide="ignore", invalid="ignore"):
            delta_r = f32(f32(dist1 - dist3) / f32(f32(2.0) * f32(f32(dist1 + dist3) - f32(f32(2.0) * dist2))))
        if delta_r < -1 or delta_r > 1:                                              # :800
            trace["outcome"][iL] = DELTA_RANGE
            continue
        best_uR = f32(scale[level_l] * f32(f32(scaled_uR0 + f32(bestinc)) + delta_r))   # :804
        disparity = f32(uL - best_uR)                                                # :806
        if disparity >= min_d and disparity < max_d:                                 # :808
            trace["outcome"][iL] = ACCEPTED
            if disparity <= 0:                                                       # :810-814
                disparity = f32(0.01)
                best_uR = f32(float(uL) - 0.01)
                trace["outcome"][iL] = CLAMPED
            depth[iL] = f32(f32(mbf) / disparity)                                    # :815-817
            uright[iL] = best_uR
            v_dist_idx.append((best_dist2, iL))
            trace["sad"][iL] = best_dist2
        else:
            trace["outcome"][iL] = DISPARITY_RANGE
    if not v_dist_idx:
        return uright, depth, 0, trace
    v_dist_idx.sort()                                                                # :822-824
    median = f32(v_dist_idx[len(v_dist_idx) // 2][0])
    th_dist = f32(f32(f32(1.5) * f32(1.4)) * median)
    trace["median"], trace["th_dist"] = float(median), float(th_dist)
    nmatched = len(v_dist_idx)
    for d, iL in reversed(v_dist_idx):                                               # :826-835
        if f32(d) < th_dist:
            break
        uright[iL] = -1
        depth[iL] = -1
        trace["outcome"][iL] = CUT
        nmatched -= 1
    return uright, depth, nmatched, trace
