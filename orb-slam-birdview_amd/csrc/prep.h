// The fisheye driver's input (prep.hip): the resident crop-and-mask handle and the launchers the other translation
// units call.  The definitions the host twins and the kernels share are prep_def.h.
#pragma once
#include "orbgpu_ctx.h"
#include "prep_def.h"

namespace orbgpu {

// k_front_prep over nframes frames.  d_crop is the crop's first byte in frame 0 (the source base plus cy * stride +
// cx * channels: orb_extract_fisheye uploads the crop alone and passes its base).  Arguments checked by the caller;
// nframes >= 1, the crop not empty, the handle on the stream's device.
hipError_t launch_front_prep(const orb_prep& p, int code, const uint8_t* d_crop, int nframes, size_t src_frame_pitch,
                             size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch, size_t dst_row_stride,
                             hipStream_t stream);

}  // namespace orbgpu

// One camera's crop and mask resident on the device (the object behind the opaque orb_prep*).  The mask is reduced
// once to the keep plane of prep_def.h over the crop: 4 bits per output pixel, one 16-bit word per lane of k_front_prep
// ((ch / 2) * quads words, 190 KB for the driver's 1900 x 800 crop).  No mask: no plane.
struct orb_prep {
    int device = 0;
    int sw = 0, sh = 0;
    int cx = 0, cy = 0, cw = 0, ch = 0;
    int quads = 0;                       // ceil(cw / 2 / 4)
    orbgpu::DevBuf<uint16_t> d_keep;   // empty without a mask
};
