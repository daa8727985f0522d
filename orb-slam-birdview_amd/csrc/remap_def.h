// cv::remap and cv::initUndistortRectifyMap as the stereo examples call them, pinned to OpenCV 3.2 on x86-64 without
// IPP: the definitions, shared by the host twins (orb_remap_host, orb_rectify_maps_host), the map
// conversion of orb_rectify_create and k_remap.  This header names no HIP symbol and compiles with a plain host
// compiler (tests/cpp_remap builds it under ASan + UBSan); build it without contraction.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ORBGPU_HD __host__ __device__
#else
#define ORBGPU_HD
#endif

namespace orbgpu {

// A map position in 1/32 pixel: OpenCV 3.2 remap's _mm_cvtps_epi32(map * 32) (imgwarp.cpp RemapInvoker).
// The product is exact or overflows; rounding is to nearest, ties to even (the default mode: std::nearbyint); NaN, an
// infinity or a product outside int give the "integer indefinite" INT_MIN.
inline int remap_fixed(float m) {
    const float p = m * 32.0f;
    if (!(p >= -2147483648.0f && p < 2147483648.0f)) return INT_MIN;
    return (int)std::nearbyint(p);
}

// The position as the kernel keeps it: the tap's corner saturated to short and the two 5-bit fractions.
struct RemapTap {
    int ix, iy;      // sat_s16(s >> 5), arithmetic shift
    unsigned frac;   // fy * 32 + fx
};

inline RemapTap remap_tap(float mx, float my) {
    const int sx = remap_fixed(mx), sy = remap_fixed(my);
    const auto sat = [](int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; };
    return RemapTap{sat(sx >> 5), sat(sy >> 5), (unsigned)(((sy & 31) << 5) | (sx & 31))};
}

// remapBilinear<FixedPtCast<int, uchar, 15>, RemapVec_8u, short>: the four integer weights (they sum to 32768) over the
// four taps, a tap outside the source read as 0 by the caller.  At most 255 * 32768 + 16384 < 2^24.
ORBGPU_HD inline uint32_t remap_blend(uint32_t fx, uint32_t fy, uint32_t s00, uint32_t s01, uint32_t s10,
                                                uint32_t s11) {
    const uint32_t w00 = (32u - fx) * (32u - fy) * 32u, w01 = fx * (32u - fy) * 32u, w10 = (32u - fx) * fy * 32u,
                   w11 = fx * fy * 32u;
    return (w00 * s00 + w01 * s01 + w10 * s10 + w11 * s11 + 16384u) >> 15;
}

// One source tap with its own border test (BORDER_CONSTANT, value 0)
ORBGPU_HD inline uint32_t remap_read(const uint8_t* src, size_t stride, int sw, int sh, int x, int y) {
    return ((unsigned)x < (unsigned)sw && (unsigned)y < (unsigned)sh) ? src[(size_t)y * stride + (size_t)x] : 0u;
}

// orb_remap_host's loop (arguments checked by the caller; src is not read when sw == 0 or sh == 0)
inline void remap_image_host(const uint8_t* src, int sw, int sh, size_t src_stride, const float* map_x,
                             const float* map_y, size_t map_stride, int dw, int dh, uint8_t* dst, size_t dst_stride) {
    for (int y = 0; y < dh; y++) {
        const float* mx = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(map_x) + (size_t)y * map_stride);
        const float* my = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(map_y) + (size_t)y * map_stride);
        uint8_t* d = dst + (size_t)y * dst_stride;
        for (int x = 0; x < dw; x++) {
            const RemapTap t = remap_tap(mx[x], my[x]);
            d[x] = (uint8_t)remap_blend(t.frac & 31u, t.frac >> 5, remap_read(src, src_stride, sw, sh, t.ix, t.iy),
                                        remap_read(src, src_stride, sw, sh, t.ix + 1, t.iy),
                                        remap_read(src, src_stride, sw, sh, t.ix, t.iy + 1),
                                        remap_read(src, src_stride, sw, sh, t.ix + 1, t.iy + 1));
        }
    }
}

// orb_rectify_maps_host's arithmetic (arguments checked by the caller; nD is 4, 5 or 8).  false: P33 * R is singular.
inline bool rectify_maps_build(const double* K, const double* D, int nD, const double* R, const double* P33, int w, int h,
                               float* map_x, float* map_y, size_t map_stride) {
    // iR = inverse(P33 * R): the product's sums in the order k = 0, 1, 2, the inverse as the adjugate times 1.0 / det
    double A[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = P33[3 * i] * R[j];
            s += P33[3 * i + 1] * R[3 + j];
            s += P33[3 * i + 2] * R[6 + j];
            A[3 * i + j] = s;
        }
    const double det = A[0] * (A[4] * A[8] - A[7] * A[5]) - A[1] * (A[3] * A[8] - A[6] * A[5]) +
                       A[2] * (A[3] * A[7] - A[6] * A[4]);
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    const double d = 1.0 / det;
    const double ir[9] = {(A[4] * A[8] - A[5] * A[7]) * d, (A[2] * A[7] - A[1] * A[8]) * d, (A[1] * A[5] - A[2] * A[4]) * d,
                          (A[5] * A[6] - A[3] * A[8]) * d, (A[0] * A[8] - A[2] * A[6]) * d, (A[2] * A[3] - A[0] * A[5]) * d,
                          (A[3] * A[7] - A[4] * A[6]) * d, (A[1] * A[6] - A[0] * A[7]) * d, (A[0] * A[4] - A[1] * A[3]) * d};
    const double fx = K[0], fy = K[4], u0 = K[2], v0 = K[5];
    const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = nD >= 5 ? D[4] : 0.0, k4 = nD >= 8 ? D[5] : 0.0,
                 k5 = nD >= 8 ? D[6] : 0.0, k6 = nD >= 8 ? D[7] : 0.0;
    for (int i = 0; i < h; i++) {
        float* m1 = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(map_x) + (size_t)i * map_stride);
        float* m2 = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(map_y) + (size_t)i * map_stride);
        double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
        for (int j = 0; j < w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {   // (sequential sums, as the reference's)
            const double wi = 1.0 / _w, x = _x * wi, y = _y * wi;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
            const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
            m1[j] = (float)(fx * xd + u0);
            m2[j] = (float)(fy * yd + v0);
        }
    }
    return true;
}

}  // namespace orbgpu
