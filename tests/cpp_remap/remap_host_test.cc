// Host check of csrc/remap_def.h (the arithmetic of orb_remap_host, orb_rectify_maps_host, orb_rectify_create's map
// conversion and k_remap) on the border cases: taps on and beyond every edge, positions no int or short holds, odd
// strides with padding, a source of another size, every distortion coefficient count.  Stand-alone: built with
// -fsanitize=address,undefined and run directly (tests/test_remap_host.py); every buffer is exactly as large as the
// contract says, so a read or write outside it is the sanitizer's to find.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../orb-slam-birdview_amd/csrc/remap_def.h"

using namespace orbgpu;

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            g_failed++;                                                      \
        }                                                                    \
    } while (0)

// one destination pixel of a sw x 1 source (1, 2, ..., sw) at map position (mx, 0)
static int at_x(int sw, float mx) {
    std::vector<uint8_t> src(sw);
    for (int i = 0; i < sw; i++) src[i] = (uint8_t)(10 * (i + 1));
    const float my = 0.0f;
    uint8_t out = 0xA5;
    remap_image_host(src.data(), sw, 1, sw, &mx, &my, 4, 1, 1, &out, 1);
    return out;
}

// the same down a 1 x sh column
static int at_y(int sh, float my) {
    std::vector<uint8_t> src(sh);
    for (int i = 0; i < sh; i++) src[i] = (uint8_t)(10 * (i + 1));
    const float mx = 0.0f;
    uint8_t out = 0xA5;
    remap_image_host(src.data(), 1, sh, 1, &mx, &my, 4, 1, 1, &out, 1);
    return out;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the fixed-point conversion
    CHECK(remap_fixed(1.0f) == 32 && remap_fixed(-1.0f) == -32);
    CHECK(remap_fixed(1.0f / 64) == 0 && remap_fixed(3.0f / 64) == 2 && remap_fixed(-1.0f / 64) == 0);   // ties to even
    CHECK(remap_fixed(nan) == INT_MIN && remap_fixed(inf) == INT_MIN && remap_fixed(-inf) == INT_MIN);
    CHECK(remap_fixed(1e30f) == INT_MIN && remap_fixed(-1e30f) == INT_MIN && remap_fixed(67108864.0f) == INT_MIN);
    CHECK(remap_fixed(-67108864.0f) == INT_MIN && remap_fixed(67108860.0f) == 2147483520);
    const RemapTap big = remap_tap(4e4f, -4e4f), indef = remap_tap(nan, inf);
    CHECK(big.ix == 32767 && big.iy == -32768 && indef.ix == -32768 && indef.iy == -32768 && indef.frac == 0);
    // the weights sum to 32768 and a constant source comes back for every fraction
    for (uint32_t fy = 0; fy < 32; fy++)
        for (uint32_t fx = 0; fx < 32; fx++) CHECK(remap_blend(fx, fy, 255, 255, 255, 255) == 255 && remap_blend(fx, fy, 0, 0, 0, 0) == 0);

    const int sw = 5;
    CHECK(at_x(sw, 0.0f) == 10 && at_x(sw, 4.0f) == 50 && at_x(sw, 0.5f) == 15);
    CHECK(at_x(sw, -0.5f) == 5);            // (S[0] + 1) >> 1
    CHECK(at_x(sw, 4.5f) == 25);            // (S[sw-1] + 1) >> 1
    for (float v : {5.0f, -1.0f, 4e4f, -4e4f, 1e30f, -1e30f, nan, inf, -inf}) {
        CHECK(at_x(sw, v) == 0);
        CHECK(at_y(sw, v) == 0);
    }
    CHECK(at_y(sw, -0.5f) == 5 && at_y(sw, 4.5f) == 25 && at_y(sw, 4.0f) == 50);

    // an empty source: every tap is outside, the source pointer is never read
    {
        const float mx[2] = {0.0f, 1.5f}, my[2] = {0.0f, 0.0f};
        uint8_t out[2] = {7, 7};
        remap_image_host(nullptr, 0, 0, 0, mx, my, 8, 2, 1, out, 2);
        CHECK(out[0] == 0 && out[1] == 0);
    }

    // odd strides, exact buffers, a source of another size: a map sweeping across all four edges and the corners
    {
        const int w = 7, h = 5, dw = 11, dh = 9;
        const size_t ss = 9, ds = 13, ms = 48;
        std::vector<uint8_t> src((h - 1) * ss + w), dst((dh - 1) * ds + dw, 0xA5);
        for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)(37 * i + 11);
        std::vector<uint8_t> mxb((dh - 1) * ms + dw * 4), myb(mxb.size());
        for (int y = 0; y < dh; y++)
            for (int x = 0; x < dw; x++) {
                const float fx = -2.0f + x * 1.03125f, fy = -2.0f + y * 1.0625f;
                std::memcpy(&mxb[y * ms + 4 * x], &fx, 4);
                std::memcpy(&myb[y * ms + 4 * x], &fy, 4);
            }
        remap_image_host(src.data(), w, h, ss, reinterpret_cast<const float*>(mxb.data()),
                         reinterpret_cast<const float*>(myb.data()), ms, dw, dh, dst.data(), ds);
        for (int y = 0; y + 1 < dh; y++)
            for (size_t x = dw; x < ds; x++) CHECK(dst[y * ds + x] == 0xA5);   // the padding keeps the sentinel
        CHECK(dst[0] == 0);                                // (-2, -2): all four taps outside
        CHECK(dst[2 * ds + 2] != 0xA5);
    }

    // the map builder: the identity calibration is the pixel grid; every coefficient count runs; singular is refused
    {
        const double K[9] = {458.654, 0, 367.215, 0, 457.296, 248.375, 0, 0, 1}, I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        const double Z[8] = {0, 0, 0, 0, 0, 0, 0, 0}, D[8] = {-0.28, 0.07, 0.0002, 1.8e-5, 0.01, 0.001, -0.002, 0.0005};
        const int w = 40, h = 30;
        std::vector<float> mx((size_t)w * h), my(mx.size());
        CHECK(rectify_maps_build(K, Z, 4, I, K, w, h, mx.data(), my.data(), (size_t)w * 4));
        int off = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) off += std::fabs(mx[y * w + x] - x) > 1e-3f || std::fabs(my[y * w + x] - y) > 1e-3f;
        CHECK(off == 0);
        for (int nD : {4, 5, 8}) {
            CHECK(rectify_maps_build(K, D, nD, I, K, w, h, mx.data(), my.data(), (size_t)w * 4));
            CHECK(std::isfinite(mx[0]) && std::isfinite(my[(size_t)w * h - 1]));
        }
        const double S[9] = {1, 2, 3, 2, 4, 6, 0, 0, 1};
        CHECK(!rectify_maps_build(K, D, 4, I, S, w, h, mx.data(), my.data(), (size_t)w * 4));
    }
    if (g_failed) return 1;
    std::printf("remap_def OK\n");
    return 0;
}
