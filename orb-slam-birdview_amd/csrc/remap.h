// cv::remap for the stereo rectification (remap.hip): the resident map handle and the launchers the other translation
// units call.  The fixed-point definition the host twin and the kernel share is remap_def.h.
#pragma once
#include "orbgpu_ctx.h"
#include "remap_def.h"

namespace orbgpu {

// At most this many maps in one launch (their pointers travel as kernel arguments)
constexpr int kRemapMaxMaps = ORB_REMAP_MAX_MAPS;

// k_remap over nframes frames, frame f through d_maps[f % nmaps] (arguments checked by the caller; nframes, dw, dh >= 1,
// 1 <= nmaps <= kRemapMaxMaps, every map of size dw x dh on the stream's device)
hipError_t launch_remap(int nmaps, const orb_rectify* const* maps, const uint8_t* d_src, int nframes, int sw, int sh,
                        size_t src_frame_pitch, size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch,
                        size_t dst_row_stride, hipStream_t stream);

}  // namespace orbgpu

// A rectification map resident on the device (the object behind the opaque orb_rectify*): the float maps converted
// once to the fixed-point form k_remap reads, as two planes in one allocation.  Rows are mpitch pixels apart (dw
// rounded up to 4, the padding zero), so a lane's four pixels are one 16-byte and one 8-byte load, both aligned:
//   plane 0  dh * mpitch dwords   iy << 16 | (ix & 0xFFFF)
//   plane 1  dh * mpitch ushorts  fy * 32 + fx
struct orb_rectify {
    int device = 0;
    int dw = 0, dh = 0;
    int mpitch = 0;
    orbgpu::DevBuf<uint32_t> d_map;   // plane 0, then plane 1
};
