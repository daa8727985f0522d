// cvtColor(..., CV_{RGB,BGR,RGBA,BGRA}2GRAY) of OpenCV 3.2 on x86-64 without IPP: the definition, shared
// by k_to_gray and orb_to_gray_host (rgbd.hip) and by the fisheye driver's front-image chain (prep_def.h).  This header
// names no HIP symbol and compiles with a plain host compiler.
#pragma once
#include <cstdint>

#include "../../include/orbgpu.h"

#ifndef ORBGPU_HD
#if defined(__HIPCC__)
#define ORBGPU_HD __host__ __device__
#else
#define ORBGPU_HD
#endif
#endif

namespace orbgpu {

// OpenCV 3.2 RGB2Gray<uchar> (color.cpp: R2Y 4899, G2Y 9617, B2Y 1868, yuv_shift 14).  c0 / c2 are
// the first and third byte of the pixel, w0 / w2 their weights (4899, 1868 for RGB*, 1868, 4899 for BGR*).  The
// weights sum to 16384 and the largest sum is 255 * 16384 + 8192 < 2^23: 24-bit multiply-adds are exact.
ORBGPU_HD inline uint32_t gray_of(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t w0, uint32_t w2) {
    return (w0 * c0 + 9617u * c1 + w2 * c2 + 8192u) >> 14;
}

inline void gray_weights(int code, uint32_t& w0, uint32_t& w2) {
    const bool bgr = code == ORB_COLOR_BGR || code == ORB_COLOR_BGRA;
    w0 = bgr ? 1868u : 4899u;
    w2 = bgr ? 4899u : 1868u;
}

}  // namespace orbgpu
