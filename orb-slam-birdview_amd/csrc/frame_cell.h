// The cell of a keypoint in the 64 x 48 Frame grid: Frame::PosInGrid (Frame.cc:549-559) as AssignFeaturesToGrid uses
// it (:378-413), for the GPU kernel (k_frame_grid, frame.hip) and for host code alike, so a CPU test compiles the
// lines the kernel runs.  No HIP header is needed: a host compiler sees a plain inline function.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ORBGPU_HD __host__ __device__
#else
#define ORBGPU_HD
#endif

namespace orbgpu {

constexpr int kCellGridCols = 64;   // FRAME_GRID_COLS (Frame.h:40)
constexpr int kCellGridRows = 48;   // FRAME_GRID_ROWS (Frame.h:39)

// posX = round((x - mnMinX) * mfGridElementWidthInv), posY likewise, in float, rounding half away from zero; the
// product of a difference has no fused form, so the value does not depend on the contraction mode.  The bounds are
// compared in float after the rounding: -0.3 rounds to -0 and lies in cell 0, and a NaN or a value no int holds falls
// out without an undefined conversion.  Returns ix * 48 + iy, or -1 for a keypoint outside the grid.
ORBGPU_HD inline int frame_cell(float x, float y, float min_x, float min_y, float inv_w, float inv_h) {
    const float fx = roundf((x - min_x) * inv_w);
    const float fy = roundf((y - min_y) * inv_h);
    if (!(fx >= 0.0f && fx < (float)kCellGridCols && fy >= 0.0f && fy < (float)kCellGridRows)) return -1;
    return (int)fx * kCellGridRows + (int)fy;
}

}  // namespace orbgpu
