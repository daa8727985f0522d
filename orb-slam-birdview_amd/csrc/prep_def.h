// The mono_fisheye driver's image path in front of System::TrackMonocularWithBirdview (Examples/Monocular/
// mono_fisheye.cc:94-116, :202-212, :244-271) and the cvtColor that Tracking::GrabImageMonocularWithBirdview opens with
// (Tracking.cc:278-307), pinned to OpenCV 3.2 on x86-64 without IPP: the definitions, shared by the host
// twins (orb_front_prep_host, orb_bird_mask_host), the keep plane of orb_prep_create and the kernels k_front_prep and
// k_bird_mask.  This header names no HIP symbol and compiles with a plain host compiler (tests/cpp_prep builds it under
// ASan + UBSan).
#pragma once
#include <cstddef>
#include <cstdint>

#include "gray_def.h"

namespace orbgpu {

// Bytes per pixel of a front-image code: 1 for ORB_PREP_GRAY, 3 or 4 for an ORB_COLOR_* code, 0 for an unknown one
inline int prep_channels(int code) {
    return code == ORB_PREP_GRAY                             ? 1
           : code == ORB_COLOR_RGB || code == ORB_COLOR_BGR   ? 3
           : code == ORB_COLOR_RGBA || code == ORB_COLOR_BGRA ? 4
                                                              : 0;
}

// applyMask (mono_fisheye.cc:202-212): a source pixel is zeroed where its mask byte (G of a 3-channel mask) is > 250
ORBGPU_HD inline bool prep_masked(uint32_t mask_byte) { return mask_byte > 250u; }

// The keep bits of one 2x2 source block: bit 0 S00, bit 1 S01 (the next column), bit 2 S10 (the next row), bit 3 S11;
// set where the pixel stays.  (sx, sy) is S00 in SOURCE coordinates; mask NULL: every pixel stays.
inline uint32_t prep_keep_bits(const uint8_t* mask, int mask_channels, size_t mask_stride, int sx, int sy) {
    if (!mask) return 15u;
    const size_t mc = (size_t)mask_channels, o = mask_channels == 3 ? 1 : 0;
    const uint8_t* m0 = mask + (size_t)sy * mask_stride + (size_t)sx * mc + o;
    const uint8_t* m1 = m0 + mask_stride;
    return (prep_masked(m0[0]) ? 0u : 1u) | (prep_masked(m0[mc]) ? 0u : 2u) | (prep_masked(m1[0]) ? 0u : 4u) |
           (prep_masked(m1[mc]) ? 0u : 8u);
}

// cv::resize(im, im, Size(0, 0), 0.5, 0.5) of one channel of one 2x2 block: for an exact factor of 2 INTER_LINEAR takes
// the INTER_AREA fast path, (S00 + S01 + S10 + S11 + 2) >> 2.  A masked pixel is a 0 in the sum, not left out of it.
ORBGPU_HD inline uint32_t prep_mean(uint32_t s00, uint32_t s01, uint32_t s10, uint32_t s11, uint32_t keep) {
    return (s00 * (keep & 1u) + s01 * ((keep >> 1) & 1u) + s10 * ((keep >> 2) & 1u) + s11 * (keep >> 3) + 2u) >> 2;
}

// One output pixel from its 2x2 block of C-channel pixels.  get(r, i) is byte i of the block's 2 * C bytes in row r of
// the block.  Every channel is averaged on its own, then (C = 3, 4) the three averaged channels go through cvtColor:
// resize first, convert second, as the reference orders them.  Alpha is not read.
template <int C, class Get>
ORBGPU_HD inline uint32_t prep_pixel(const Get& get, uint32_t keep, uint32_t w0, uint32_t w2) {
    if constexpr (C == 1) {
        return prep_mean(get(0, 0), get(0, 1), get(1, 0), get(1, 1), keep);
    } else {
        const uint32_t m0 = prep_mean(get(0, 0), get(0, C), get(1, 0), get(1, C), keep);
        const uint32_t m1 = prep_mean(get(0, 1), get(0, C + 1), get(1, 1), get(1, C + 1), keep);
        const uint32_t m2 = prep_mean(get(0, 2), get(0, C + 2), get(1, 2), get(1, C + 2), keep);
        return gray_of(m0, m1, m2, w0, w2);
    }
}

// get() over the two rows of a block in memory
struct PrepBytes {
    const uint8_t* r0;
    const uint8_t* r1;
    ORBGPU_HD uint32_t operator()(int r, int i) const { return (r ? r1 : r0)[i]; }
};

// orb_front_prep_host's loop (arguments checked by the caller): the (cw / 2) x (ch / 2) gray image of the crop
// (cx, cy, cw, ch) of src, cw and ch even
template <int C>
inline void front_prep_image_host(const uint8_t* src, size_t src_stride, const uint8_t* mask, int mask_channels,
                                  size_t mask_stride, int cx, int cy, int cw, int ch, uint32_t w0, uint32_t w2,
                                  uint8_t* dst, size_t dst_stride) {
    for (int oy = 0; oy < ch / 2; oy++) {
        const int sy = cy + 2 * oy;
        const uint8_t* r0 = src + (size_t)sy * src_stride;
        uint8_t* d = dst + (size_t)oy * dst_stride;
        for (int ox = 0; ox < cw / 2; ox++) {
            const int sx = cx + 2 * ox;
            const PrepBytes get{r0 + (size_t)sx * C, r0 + src_stride + (size_t)sx * C};
            d[ox] = (uint8_t)prep_pixel<C>(get, prep_keep_bits(mask, mask_channels, mask_stride, sx, sy), w0, w2);
        }
    }
}

// The keep plane orb_prep_create keeps on the device: one 16-bit word per (output row, quad of output pixels), the
// keep bits of output pixel 4 q + k in bits [4 k, 4 k + 4); pixels past the row's end read 0.  plane: (ch / 2) * quads
// words, quads = ceil(cw / 2 / 4).
inline void prep_keep_plane(const uint8_t* mask, int mask_channels, size_t mask_stride, int cx, int cy, int cw, int ch,
                            uint16_t* plane) {
    const int ow = cw / 2, oh = ch / 2, quads = (ow + 3) / 4;
    for (int oy = 0; oy < oh; oy++)
        for (int q = 0; q < quads; q++) {
            uint32_t v = 0;
            for (int k = 0; k < 4 && 4 * q + k < ow; k++)
                v |= prep_keep_bits(mask, mask_channels, mask_stride, cx + 2 * (4 * q + k), cy + 2 * oy) << (4 * k);
            plane[(size_t)oy * quads + q] = (uint16_t)v;
        }
}

// ConvertMaskBirdview (mono_fisheye.cc:244-271) before its footprint: 0 where G < 20, else 250 (not 255)
ORBGPU_HD inline uint32_t bird_mask_value(uint32_t g) { return g < 20u ? 0u : 250u; }

// orb_bird_mask_host's conversion loop (arguments checked by the caller; C is 3 or 4); the footprint is the caller's
inline void bird_mask_convert_host(int C, const uint8_t* src, int w, int h, size_t src_stride, uint8_t* dst,
                                   size_t dst_stride) {
    for (int y = 0; y < h; y++) {
        const uint8_t* s = src + (size_t)y * src_stride;
        uint8_t* d = dst + (size_t)y * dst_stride;
        for (int x = 0; x < w; x++) d[x] = (uint8_t)bird_mask_value(s[(size_t)x * C + 1]);
    }
}

}  // namespace orbgpu
