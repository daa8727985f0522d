// Colour input and the RGB-D depth gather (rgbd.hip): the launchers the other translation units call.
#pragma once
#include "orbgpu_ctx.h"

namespace orbgpu {

// Bytes per pixel of an ORB_COLOR_* code (3 or 4), 0 for an unknown code
inline int color_channels(int code) {
    return code == ORB_COLOR_RGB || code == ORB_COLOR_BGR ? 3 : code == ORB_COLOR_RGBA || code == ORB_COLOR_BGRA ? 4 : 0;
}

// k_to_gray over nframes frames (arguments checked by the caller; nframes, w, h >= 1)
hipError_t launch_to_gray(int code, const uint8_t* d_src, int nframes, int w, int h, size_t src_frame_pitch,
                          size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch, size_t dst_row_stride,
                          hipStream_t stream);

// k_rgbd_depth over a batch in orb_extract_batch_device's output layout; map.data is device memory; d_nvalid may be
// nullptr.  Arguments checked by the caller; nframes >= 1.
hipError_t launch_rgbd_depth(const orb_depth_map& map, float mbf, int nframes, const orb_keypoint* d_raw,
                             const orb_keypoint* d_un, const int* d_counts, int kp_cap, float* d_uright, float* d_depth,
                             int* d_nvalid, hipStream_t stream);

}  // namespace orbgpu
