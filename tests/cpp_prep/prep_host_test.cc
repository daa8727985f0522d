// The definitions of csrc/prep_def.h at their edge sizes, in exactly-sized heap buffers so that ASan sees any byte read or
// written outside the crop rows' [cx * C, (cx + cw) * C) or the destination's [row, row + cw / 2):
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined prep_host_test.cc && ./a.out
// (built and run by tests/test_prep_host.py).  Prints "prep_def OK".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../orb-slam-birdview_amd/csrc/prep_def.h"

using namespace orbgpu;

namespace {

int failures = 0;
#define EXPECT(c)                                                    \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            failures++;                                              \
        }                                                            \
    } while (0)

uint32_t lcg = 12345;
uint8_t rnd() {
    lcg = lcg * 1664525u + 1013904223u;
    return (uint8_t)(lcg >> 24);
}

// a plain second statement of one output pixel, for the comparison
uint32_t expect_pixel(int C, const uint8_t* src, size_t stride, const uint8_t* mask, int mc, size_t ms, int sx, int sy,
                      uint32_t w0, uint32_t w2) {
    uint32_t m[3] = {0, 0, 0};
    for (int c = 0; c < (C == 1 ? 1 : 3); c++) {
        uint32_t s = 2;
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const bool gone = mask && mask[(size_t)(sy + dy) * ms + (size_t)(sx + dx) * mc + (mc == 3 ? 1 : 0)] > 250;
                if (!gone) s += src[(size_t)(sy + dy) * stride + (size_t)(sx + dx) * C + c];
            }
        m[c] = s >> 2;
    }
    return C == 1 ? m[0] : (w0 * m[0] + 9617u * m[1] + w2 * m[2] + 8192u) >> 14;
}

template <int C>
void run_case(int sw, int sh, int cx, int cy, int cw, int ch, int mc, int code) {
    // exactly sized: the last row ends at its last byte
    const size_t stride = (size_t)sw * C, ms = (size_t)sw * (mc ? mc : 1);
    std::vector<uint8_t> src(stride * sh), mask(mc ? ms * sh : 0);
    for (auto& b : src) b = rnd();
    for (auto& b : mask) b = (uint8_t)(248 + rnd() % 8);
    const int ow = cw / 2, oh = ch / 2;
    std::vector<uint8_t> dst((size_t)ow * oh, 0xA5);
    uint32_t w0 = 0, w2 = 0;
    gray_weights(code, w0, w2);
    const uint8_t* mp = mc ? mask.data() : nullptr;
    front_prep_image_host<C>(src.data(), stride, mp, mc, ms, cx, cy, cw, ch, w0, w2, dst.data(), (size_t)ow);
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++)
            EXPECT(dst[(size_t)y * ow + x] ==
                   expect_pixel(C, src.data(), stride, mp, mc, ms, cx + 2 * x, cy + 2 * y, w0, w2));
    // the keep plane the device form reads, against the same mask
    const int quads = (ow + 3) / 4;
    std::vector<uint16_t> plane((size_t)quads * oh, 0xFFFF);
    prep_keep_plane(mp, mc, ms, cx, cy, cw, ch, plane.data());
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < 4 * quads; x++) {
            const uint32_t bits = (plane[(size_t)y * quads + x / 4] >> (4 * (x % 4))) & 15u;
            EXPECT(bits == (x < ow ? prep_keep_bits(mp, mc, ms, cx + 2 * x, cy + 2 * y) : 0u));
        }
}

template <int C>
void run_sizes(int code) {
    for (int mc : {0, 1, 3}) {
        run_case<C>(2, 2, 0, 0, 2, 2, mc, code);        // a 2 x 2 crop of a 2 x 2 source
        run_case<C>(7, 5, 5, 3, 2, 2, mc, code);        // a 2 x 2 crop flush with the last row and column
        run_case<C>(13, 9, 3, 1, 10, 8, mc, code);      // flush with both, an odd cx, output width 5
        run_case<C>(70, 40, 0, 0, 70, 40, mc, code);    // the whole source
        run_case<C>(9, 4, 1, 0, 0, 4, mc, code);        // an empty crop: nothing read, nothing written
    }
}

}  // namespace

int main() {
    EXPECT(prep_channels(ORB_PREP_GRAY) == 1 && prep_channels(ORB_COLOR_BGR) == 3 && prep_channels(ORB_COLOR_RGBA) == 4);
    EXPECT(prep_channels(4) == 0 && prep_channels(-2) == 0);
    EXPECT(!prep_masked(250) && prep_masked(251));
    EXPECT(prep_mean(1, 1, 0, 0, 15) == 1 && prep_mean(1, 0, 0, 0, 15) == 0 && prep_mean(255, 255, 255, 255, 15) == 255);
    EXPECT(prep_mean(100, 100, 100, 100, 14) == 75 && prep_mean(9, 9, 9, 9, 0) == 0);
    EXPECT(bird_mask_value(19) == 0 && bird_mask_value(20) == 250 && bird_mask_value(255) == 250);
    run_sizes<1>(ORB_PREP_GRAY);
    run_sizes<3>(ORB_COLOR_BGR);
    run_sizes<3>(ORB_COLOR_RGB);
    run_sizes<4>(ORB_COLOR_BGRA);
    run_sizes<4>(ORB_COLOR_RGBA);
    // ConvertMaskBirdview's loop in exactly sized buffers, 3 and 4 channels, 1 x 1 included
    for (int C : {3, 4})
        for (int w : {1, 5, 64}) {
            const int h = 3;
            std::vector<uint8_t> src((size_t)w * h * C), dst((size_t)w * h, 0xA5);
            for (auto& b : src) b = (uint8_t)(rnd() % 40);
            bird_mask_convert_host(C, src.data(), w, h, (size_t)w * C, dst.data(), (size_t)w);
            for (int i = 0; i < w * h; i++) EXPECT(dst[i] == (src[(size_t)i * C + 1] < 20 ? 0 : 250));
        }
    if (failures) return fprintf(stderr, "%d failures\n", failures), 1;
    printf("prep_def OK\n");
    return 0;
}
