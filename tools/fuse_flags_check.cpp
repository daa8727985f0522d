// Built with -ffp-contract=off and linked with tools/fuse_flags_probe.cpp (built with the reference's
// -O3 -march=native -std=c++11).  Checks that the explicit float forms of Fuse's reprojection gate that
// fuse_gate_skips (csrc/grid_window.h: the one definition k_projection_best and orb_project_best_host compile, called
// here for the verdict) and tests/kf_projection_ref.py use are the ones GCC produces for the reference's expressions
// (ORBmatcher.cc:914-938):
//   stereo  e2 = fmaf(er, er, fmaf(ex, ex, ey * ey)),   skipped when (double)(e2 * invSigma2) > 7.8
//   mono    e2 = fmaf(ex, ex, ey * ey),                 skipped when (double)(e2 * invSigma2) > 5.99
// and how often the uncontracted sums would differ.
//   fuse_flags_check [cases]        one JSON object; exit status 1 on any mismatch
//   fuse_flags_check dump <cases>   per case a line of hex float bits "u v ur kpx kpy kpr inv e2 skipped" with the
//                                   probe's e2 and verdict (for the test-side fmaf helper)
// Test infrastructure (tests/test_fuse_flags.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../orb-slam-birdview_amd/csrc/grid_window.h"   // (relative to this file: the compile line needs no -I)

namespace fuse_probe {
struct KeyPoint { float x, y; int octave; };
void fuse_gate(float u, float v, float ur, int n, const KeyPoint* mvKeysUn, const float* mvuRight,
               const float* mvInvLevelSigma2, float* e2_out, unsigned char* skipped);
}  // namespace fuse_probe

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    const bool dump = argc > 2 && !std::strcmp(argv[1], "dump");
    const long cases = dump ? std::atol(argv[2]) : (argc > 1 ? std::atol(argv[1]) : 1000000);
    std::mt19937 rng(20240607);
    std::uniform_real_distribution<float> P(0.f, 640.f), D(-6.f, 6.f), R(0.f, 1.f);
    float inv[8];   // mvInvLevelSigma2 of scaleFactor 1.2 (ORBextractor.cc:431-447)
    {
        float s = 1.0f, sigma2[8];
        for (int i = 0; i < 8; i++) {
            sigma2[i] = s * s;
            inv[i] = 1.0f / sigma2[i];
            s = s * 1.2f;
        }
    }
    const int N = 64;   // candidates per probe call (a loop, as in the reference)
    std::vector<fuse_probe::KeyPoint> kps(N);
    std::vector<float> uright(N), e2(N);
    std::vector<unsigned char> skipped(N);
    long n = 0, nstereo = 0, bad_e2 = 0, bad_skip = 0, sep_e2 = 0, sep_skip = 0, nskipped = 0;
    while (n < cases) {
        const float u = P(rng), v = P(rng) * 0.75f, ur = u - 40.f * (0.01f + 0.09f * R(rng));
        for (int i = 0; i < N; i++) {
            const float spread = (i & 3) == 0 ? 0.2f : 1.f;   // a quarter close to the projection
            kps[i].x = u + D(rng) * spread;
            kps[i].y = v + D(rng) * spread;
            kps[i].octave = (int)(rng() & 7);
            const uint32_t k = rng() % 10;
            uright[i] = k < 4 ? -1.f : (k == 4 ? 0.f : ur + D(rng) * spread);
        }
        fuse_probe::fuse_gate(u, v, ur, N, kps.data(), uright.data(), inv, e2.data(), skipped.data());
        for (int i = 0; i < N && n < cases; i++, n++) {
            const float ex = u - kps[i].x, ey = v - kps[i].y, er = ur - uright[i];
            const bool stereo = uright[i] >= 0;
            const float is2 = inv[kps[i].octave];
            float want, sep;
            bool skip_sep;
            // the verdict is the library's own function; e2 is written out here for the bit comparison
            const bool skip = orbgpu::fuse_gate_skips(u, v, ur, kps[i].x, kps[i].y, uright[i], is2);
            if (stereo) {
                want = std::fmaf(er, er, std::fmaf(ex, ex, ey * ey));
                sep = ex * ex + ey * ey + er * er;
                skip_sep = (double)(sep * is2) > 7.8;
            } else {
                want = std::fmaf(ex, ex, ey * ey);
                sep = ex * ex + ey * ey;
                skip_sep = (double)(sep * is2) > 5.99;
            }
            nstereo += stereo;
            nskipped += skipped[i];
            bad_e2 += bits(want) != bits(e2[i]);
            bad_skip += skip != (skipped[i] != 0);
            sep_e2 += bits(sep) != bits(want);
            sep_skip += skip_sep != skip;
            if (dump)
                std::printf("%08x %08x %08x %08x %08x %08x %08x %08x %d\n", bits(u), bits(v), bits(ur), bits(kps[i].x),
                            bits(kps[i].y), bits(uright[i]), bits(is2), bits(e2[i]), (int)skipped[i]);
        }
    }
    if (!dump)
        std::printf("{\"cases\": %ld, \"stereo_cases\": %ld, \"skipped\": %ld, \"e2_mismatch\": %ld, "
                    "\"skip_mismatch\": %ld, \"e2_uncontracted_differs\": %ld, \"skip_uncontracted_differs\": %ld}\n",
                    n, nstereo, nskipped, bad_e2, bad_skip, sep_e2, sep_skip);
    return (bad_e2 || bad_skip) ? 1 : 0;
}
