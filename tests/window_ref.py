"""Plain Python restatements, written from the reference source, of the window matchers:
ORBmatcher::SearchForInitialization (ORBmatcher.cc:405-520; level0_only) and BirdviewMatch(const Frame&, const
Frame&, ...) (:1788-1899; every level), with Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:378-393, :549-559) and
Frame::GetFeaturesInArea (:494-547) in float32.  The matcher returns a trace with one record per feature of F1."""
import numpy as np

from bow_ref import HISTO_LENGTH, TH_LOW, c_round, descriptor_distance, rot_bin, three_maxima

f32 = np.float32
COLS, ROWS = 64, 48
INT_MAX = 2 ** 31 - 1
LEVEL, EMPTY, DIST, RATIO, ACCEPTED = "level above 0", "empty window", "bestDist above TH_LOW", "ratio test", "accepted"


class Grid:
    """mGrid[ix][iy] of a frame with bounds (min_x, max_x, min_y, max_y)."""

    def __init__(self, kps, min_x, max_x, min_y, max_y):
        self.kps, self.min_x, self.min_y = kps, f32(min_x), f32(min_y)
        self.inv_w = f32(f32(COLS) / f32(f32(max_x) - f32(min_x)))
        self.inv_h = f32(f32(ROWS) / f32(f32(max_y) - f32(min_y)))
        self.cells = [[[] for _ in range(ROWS)] for _ in range(COLS)]
        for i in range(len(kps)):
            px = c_round(f32(f32(f32(kps["x"][i]) - self.min_x) * self.inv_w))
            py = c_round(f32(f32(f32(kps["y"][i]) - self.min_y) * self.inv_h))
            if px < 0 or px >= COLS or py < 0 or py >= ROWS:
                continue
            self.cells[px][py].append(i)

    def csr(self):
        """(inv_w, inv_h, cell_off, cell_idx): cell (ix, iy) at ix * ROWS + iy."""
        off, idx = [0], []
        for ix in range(COLS):
            for iy in range(ROWS):
                idx += self.cells[ix][iy]
                off.append(len(idx))
        return float(self.inv_w), float(self.inv_h), np.array(off, np.int32), np.array(idx, np.int32)

    def features_in_area(self, x, y, r, min_level, max_level):
        x, y, r = f32(x), f32(y), f32(r)
        out = []
        x0 = max(0, int(np.floor(f32(f32(f32(x - self.min_x) - r) * self.inv_w))))
        if x0 >= COLS:
            return out
        x1 = min(COLS - 1, int(np.ceil(f32(f32(f32(x - self.min_x) + r) * self.inv_w))))
        if x1 < 0:
            return out
        y0 = max(0, int(np.floor(f32(f32(f32(y - self.min_y) - r) * self.inv_h))))
        if y0 >= ROWS:
            return out
        y1 = min(ROWS - 1, int(np.ceil(f32(f32(f32(y - self.min_y) + r) * self.inv_h))))
        if y1 < 0:
            return out
        check = min_level > 0 or max_level >= 0
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for j in self.cells[ix][iy]:
                    kp = self.kps[j]
                    if check:
                        if kp["octave"] < min_level:
                            continue
                        if max_level >= 0 and kp["octave"] > max_level:
                            continue
                    if abs(f32(f32(kp["x"]) - x)) < r and abs(f32(f32(kp["y"]) - y)) < r:
                        out.append(j)
        return out


def candidate_lists(grid, kps1, r):
    """vIndices2 of every feature of F1 (window centre = its own position, level = its octave)."""
    return [grid.features_in_area(k["x"], k["y"], r, int(k["octave"]), int(k["octave"])) for k in kps1]


def window_match(nnratio, check_ori, level0_only, desc1, kps1, desc2, kps2, cands):
    """cands[i1] = vIndices2 of feature i1.  Returns (nmatches, vnMatches12, trace)."""
    nnratio = f32(nnratio)
    matches12 = [-1] * len(desc1)
    matched_distance = [INT_MAX] * len(desc2)
    matches21 = [-1] * len(desc2)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    visits = []
    for i1 in range(len(desc1)):
        rec = dict(i1=i1, outcome=None, d1=None, d2=None, best=-1, blocked=[], replaced=-1, ncand=len(cands[i1]))
        visits.append(rec)
        if level0_only and kps1[i1]["octave"] > 0:
            rec["outcome"] = LEVEL
            continue
        if not cands[i1]:
            rec["outcome"] = EMPTY
            continue
        best, best2, best_idx2 = INT_MAX, INT_MAX, -1
        for i2 in cands[i1]:
            dist = descriptor_distance(desc1[i1], desc2[i2])
            if matched_distance[i2] <= dist:
                rec["blocked"].append((i2, dist, matched_distance[i2]))
                continue
            if dist < best:
                best2, best, best_idx2 = best, dist, i2
            elif dist < best2:
                best2 = dist
        rec.update(d1=best, d2=best2, best=best_idx2)
        if not best <= TH_LOW:
            rec["outcome"] = DIST
            continue
        if not f32(best) < f32(f32(best2) * nnratio):
            rec["outcome"] = RATIO
            continue
        rec["outcome"] = ACCEPTED
        if matches21[best_idx2] >= 0:
            rec["replaced"] = matches21[best_idx2]
            matches12[matches21[best_idx2]] = -1
            nmatches -= 1
        matches12[i1] = best_idx2
        matches21[best_idx2] = i1
        matched_distance[best_idx2] = best
        nmatches += 1
        if check_ori:
            b, _ = rot_bin(kps1[i1]["angle"], kps2[best_idx2]["angle"])
            rot_hist[b].append(i1)
    sizes = [len(h) for h in rot_hist]
    culled = 0
    if check_ori:
        ind = three_maxima(sizes)
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for idx1 in rot_hist[i]:
                if matches12[idx1] >= 0:
                    matches12[idx1] = -1
                    nmatches -= 1
                    culled += 1
    return nmatches, np.array(matches12, np.int32), dict(visits=visits, sizes=sizes, culled=culled)
