// A search window over the 64 x 48 Frame grid: the cell rectangle and the candidate filter of
// Frame::GetFeaturesInArea (Frame.cc:494-547; KeyFrame::GetFeaturesInArea, KeyFrame.cc:585-629, is the same walk
// without levels) and Fuse's reprojection gate (ORBmatcher.cc:914-938), for the grid kernels (k_window_topk,
// k_projection_topk, k_projection_best: hamming_kernels.hip) and for host code (proj_best_one, orb_features_in_area:
// matcher.hip) alike, so a CPU test compiles the lines the kernels run (tests/cpp_grid_window, tools/fuse_flags_check.cpp).
// No HIP header is needed: a host compiler sees plain inline functions.  The translation units that include this build
// with -ffp-contract=off, so the fmaf of fuse_gate_skips are the only fused operations.
#pragma once
#include <math.h>

#include "frame_cell.h"

namespace orbgpu {

// Cells [x0, x1] x [y0, y1] of the grid, cell (ix, iy) at ix * kCellGridRows + iy; empty: the window lies wholly off
// one side and the bounds are not to be used.
struct CellRect {
    int x0, x1, y0, y1;
    bool empty;
};

// The rectangle of the window of half-width r about (x, y) (Frame.cc:499-513): the reference's float expressions, a
// sum then a product, so no fused form exists.  Precondition: finite inputs (r >= 0, inv_w and inv_h a grid's, so
// the products are values an int holds); the entry points refuse other queries (proj_queries_fault,
// bird_queries_fault: matcher.hip) before anything reaches here.
__attribute__((always_inline)) ORBGPU_HD inline CellRect cell_rect(float x, float y, float r, float min_x, float min_y,
                                                                   float inv_w, float inv_h) {
    const int fx0 = (int)floorf((x - min_x - r) * inv_w), fx1 = (int)ceilf((x - min_x + r) * inv_w);
    const int fy0 = (int)floorf((y - min_y - r) * inv_h), fy1 = (int)ceilf((y - min_y + r) * inv_h);
    CellRect c;
    c.x0 = fx0 > 0 ? fx0 : 0;
    c.x1 = fx1 < kCellGridCols - 1 ? fx1 : kCellGridCols - 1;
    c.y0 = fy0 > 0 ? fy0 : 0;
    c.y1 = fy1 < kCellGridRows - 1 ? fy1 : kCellGridRows - 1;
    c.empty = c.x0 >= kCellGridCols || c.x1 < 0 || c.y0 >= kCellGridRows || c.y1 < 0;
    return c;
}

// The box of Frame.cc:537-541: both distances strictly below r (a keypoint at exactly r is outside; r = 0 admits
// nothing).  KP is any keypoint with x, y and octave (orb_keypoint).
template <class KP>
__attribute__((always_inline)) ORBGPU_HD inline bool window_box(const KP& kp, float x, float y, float r) {
    return fabsf(kp.x - x) < r && fabsf(kp.y - y) < r;
}

// A cell's keypoint is a candidate (Frame.cc:515-541): the level range, then the box.  (min_level, max_level) as the
// reference takes them: (0, -1) and (-1, -1) check no level, max_level < 0 leaves the range open above.
// k_window_topk asks for the query's own octave lv and keeps its `octave != lv` beside window_box instead of calling
// this with (lv, lv): the two agree for every lv >= 0 (lv = 0 included: max_level = 0 >= 0 turns the check on, and
// octave < 0 or > 0 is refused), but for a query octave below 0, which no entry point refuses, (lv, lv) checks no
// level at all where the kernel admits only the equal octave.
template <class KP>
__attribute__((always_inline)) ORBGPU_HD inline bool window_admits(const KP& kp, float x, float y, float r,
                                                                   int min_level, int max_level) {
    const bool bCheckLevels = min_level > 0 || max_level >= 0;   // :515
    if (bCheckLevels) {                                          // :528-535
        if (kp.octave < min_level) return false;
        if (max_level >= 0 && kp.octave > max_level) return false;
    }
    return window_box(kp, x, y, r);
}

// Fuse's reprojection gate of the projection (u, v, ur) against a keypoint at (kp_x, kp_y) with right coordinate urt
// (< 0: monocular) and its level's inverse sigma^2 (ORBmatcher.cc:914-938): true = the candidate is skipped.  The sums
// in the reference build's contracted forms (tools/fuse_flags_probe.cpp): stereo e2 = fma(er, er, fma(ex, ex, ey ey))
// against 7.8, mono e2 = fma(ex, ex, ey ey) against 5.99, the product in float and the compare in double.  fmaf is
// exact whether it is an instruction or libm's.
__attribute__((always_inline)) ORBGPU_HD inline bool fuse_gate_skips(float u, float v, float ur, float kp_x,
                                                                     float kp_y, float urt, float inv_sigma2) {
    const float ex = u - kp_x, ey = v - kp_y;
    const float e2m = __builtin_fmaf(ex, ex, ey * ey);
    if (urt >= 0) {
        const float er = ur - urt;
        const float e2 = __builtin_fmaf(er, er, e2m);
        return (double)(e2 * inv_sigma2) > 7.8;
    }
    return (double)(e2m * inv_sigma2) > 5.99;
}

}  // namespace orbgpu
