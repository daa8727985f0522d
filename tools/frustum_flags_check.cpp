// Built with -ffp-contract=off and linked with tools/frustum_flags_probe.cpp (built with the reference's -O3
// -march=native -std=c++11).  Checks that the explicit float forms of the projection lines that k_project_points /
// orb_project_points_host (csrc/point_project.h) and tests/frustum_ref.py use are the ones GCC produces for the
// reference's expressions:
//   Frame::isInFrustum (Frame.cc:454-456, :486)   u = fmaf(fx * PcX, invz, cx), ur = fmaf(-mbf, invz, u)
//   Fuse (ORBmatcher.cc:859-870)                  x = PcX * invz, u = fmaf(fx, x, cx), ur = fmaf(-bf, invz, u)
// and how often the uncontracted forms would differ; and the level thresholds of MapPoint::PredictScale
// (MapPoint.cc:385-417) against the direct ceilf(logf(r) / lsf) clamp.
//   frustum_flags_check [cases]      one JSON object; exit status 1 on any mismatch
//   frustum_flags_check levels       the threshold check for scale factors 1.2f, 1.1f, 2.0f at 8 levels (one JSON object)
// Test infrastructure (tests/test_frustum_pin.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace frustum_probe {
struct Camera { float fx, fy, cx, cy, mbf, mnMinX, mnMaxX, mnMinY, mnMaxY; };
void frame_lines(const Camera& c, int n, const float* Pc, float* out, unsigned char* kept);
void fuse_lines(const Camera& c, int n, const float* p3Dc, float* out, unsigned char* kept);
}  // namespace frustum_probe

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// MapPoint::PredictScale's clamp of a finite positive ratio, in float before the cast
static int direct_level(float r, float lsf, int nlevels) {
    const float s = std::ceil(std::log(r) / lsf);
    if (!(s >= 0)) return 0;
    if (s >= (float)nlevels) return nlevels - 1;
    return (int)s;
}

// The library's rule: T[k] by bisection over float bit patterns with this libm's logf
static void thresholds(float lsf, int nlevels, float* T) {
    for (int k = 0; k + 1 < nlevels; k++) {
        auto above = [&](uint32_t b) { return std::ceil(std::log(from_bits(b)) / lsf) > (float)k; };
        uint32_t lo = 1, hi = 0x7f7fffffu;
        T[k] = INFINITY;
        if (!above(hi)) continue;
        if (above(lo)) {
            T[k] = from_bits(lo);
            continue;
        }
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            (above(mid) ? hi : lo) = mid;
        }
        T[k] = from_bits(hi);
    }
}

static int levels_main() {
    const float factors[3] = {1.2f, 1.1f, 2.0f};
    const int nlevels = 8;
    long near = 0, bad_near = 0, uniform = 0, bad_uniform = 0;
    std::mt19937 rng(20240611);
    std::uniform_real_distribution<float> E(-4.0f, 8.0f);
    for (float sf : factors) {
        const float lsf = std::log(sf);
        float T[16];
        thresholds(lsf, nlevels, T);
        auto counted = [&](float r) {
            int l = 0;
            for (int k = 0; k + 1 < nlevels; k++) l += r >= T[k];
            return l;
        };
        for (int k = 0; k + 1 < nlevels; k++)
            for (int d = -4096; d <= 4096; d++) {
                const float r = from_bits(bits(T[k]) + d);
                near++;
                bad_near += counted(r) != direct_level(r, lsf, nlevels);
            }
        for (long i = 0; i < 1000000; i++) {
            const float r = std::exp2(E(rng));   // log-uniform in [2^-4, 2^8]
            uniform++;
            bad_uniform += counted(r) != direct_level(r, lsf, nlevels);
        }
    }
    std::printf("{\"near_cases\": %ld, \"near_mismatch\": %ld, \"uniform_cases\": %ld, \"uniform_mismatch\": %ld}\n", near,
                bad_near, uniform, bad_uniform);
    return (bad_near || bad_uniform) ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "levels")) return levels_main();
    const long cases = argc > 1 ? std::atol(argv[1]) : 1000000;
    std::mt19937 rng(20240610);
    std::uniform_real_distribution<float> U(-100.f, 740.f), V(-80.f, 560.f), Z(0.5f, 30.f);
    const frustum_probe::Camera c{517.3f, 516.5f, 318.6f, 255.3f, 40.0f, 0.0f, 640.0f, 0.0f, 480.0f};
    const int N = 64;   // points per probe call (a loop, as in the reference)
    std::vector<float> Pc(3 * N), a(4 * N), b(4 * N);
    std::vector<unsigned char> ka(N), kb(N);
    long n = 0, kept_frame = 0, kept_fuse = 0, bad_frame = 0, bad_fuse = 0, bad_kept = 0;
    long sep_frame_u = 0, sep_frame_ur = 0, sep_fuse_u = 0, sep_fuse_ur = 0, cross_u = 0;
    while (n < cases) {
        for (int i = 0; i < N; i++) {
            const float z = (rng() % 16 == 0) ? -Z(rng) : Z(rng);
            Pc[3 * i] = (U(rng) - c.cx) / c.fx * z;
            Pc[3 * i + 1] = (V(rng) - c.cy) / c.fy * z;
            Pc[3 * i + 2] = z;
        }
        frustum_probe::frame_lines(c, N, Pc.data(), a.data(), ka.data());
        frustum_probe::fuse_lines(c, N, Pc.data(), b.data(), kb.data());
        for (int i = 0; i < N && n < cases; i++, n++) {
            const float X = Pc[3 * i], Y = Pc[3 * i + 1], Zc = Pc[3 * i + 2];
            if (Zc < 0.0f) {
                bad_kept += ka[i] != 0 || kb[i] != 0;
                continue;
            }
            const float invz = 1.0f / Zc;
            // Frame::isInFrustum
            const float u = std::fmaf(c.fx * X, invz, c.cx), v = std::fmaf(c.fy * Y, invz, c.cy);
            const bool in_a = !(u < c.mnMinX || u > c.mnMaxX) && !(v < c.mnMinY || v > c.mnMaxY);
            bad_frame += bits(u) != bits(a[4 * i]) || bits(v) != bits(a[4 * i + 1]) || bits(invz) != bits(a[4 * i + 3]);
            bad_kept += in_a != (ka[i] != 0);
            sep_frame_u += bits(c.fx * X * invz + c.cx) != bits(u);
            if (in_a) {
                const float ur = std::fmaf(-c.mbf, invz, u);
                bad_frame += bits(ur) != bits(a[4 * i + 2]);
                sep_frame_ur += bits(u - c.mbf * invz) != bits(ur);
                kept_frame++;
            }
            // Fuse
            const float x = X * invz, y = Y * invz;
            const float fu = std::fmaf(c.fx, x, c.cx), fv = std::fmaf(c.fy, y, c.cy);
            const bool in_b = fu >= c.mnMinX && fu < c.mnMaxX && fv >= c.mnMinY && fv < c.mnMaxY;
            bad_fuse += bits(fu) != bits(b[4 * i]) || bits(fv) != bits(b[4 * i + 1]) || bits(invz) != bits(b[4 * i + 3]);
            bad_kept += in_b != (kb[i] != 0);
            sep_fuse_u += bits(c.fx * x + c.cx) != bits(fu);
            cross_u += bits(fu) != bits(u);
            if (in_b) {
                const float ur = std::fmaf(-c.mbf, invz, fu);
                bad_fuse += bits(ur) != bits(b[4 * i + 2]);
                sep_fuse_ur += bits(fu - c.mbf * invz) != bits(ur);
                kept_fuse++;
            }
        }
    }
    std::printf("{\"cases\": %ld, \"kept_frame\": %ld, \"kept_fuse\": %ld, \"frame_mismatch\": %ld, \"fuse_mismatch\": %ld, "
                "\"kept_mismatch\": %ld, \"frame_u_uncontracted_differs\": %ld, \"frame_ur_uncontracted_differs\": %ld, "
                "\"fuse_u_uncontracted_differs\": %ld, \"fuse_ur_uncontracted_differs\": %ld, "
                "\"frame_u_differs_from_fuse_u\": %ld}\n",
                n, kept_frame, kept_fuse, bad_frame, bad_fuse, bad_kept, sep_frame_u, sep_frame_ur, sep_fuse_u,
                sep_fuse_ur, cross_u);
    return (bad_frame || bad_fuse || bad_kept) ? 1 : 0;
}
