// Drives the host mirror's projection-gated searches the way Tracking drives the reference's:
//   test_projection_mirror <cases.bin> <results.bin>
// cases.bin (little endian, written by tests/test_gpu_projection_mirror.py): int32 ncases, then per case
//   int32 form (0: SearchByProjection(CurrentFrame, LastFrame), 1: SearchByProjection(F, MapPoints), 2: ...Bird)
//   the Frame: int32 nt | nt keypoints (28 B) | nt descriptors (32 B) | float bounds[4] (minX, maxX, minY, maxY)
//              | int32 has_uright | nt float uright (if has_uright) | nt uint8 taken | float scale[8] | float mbf
//   float nnratio | int32 check_ori | float th (form 2: r) | int32 bMono, bForward, bBackward | int32 nq
//   form 0: nq float u, v, invzc | nq int32 octave | nq float angle | nq uint8 observed | nq descriptors
//   form 1: nq float projX, projY, projXR | nq int32 level | nq float viewCos | nq descriptors
//   form 2: nq float x, y | nq descriptors
// results.bin: per case int32 nmatches | int32 nt | nt int32 (the result vector).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../orb-slam-birdview_amd/host/ORBmatcher.h"

using namespace ORB_SLAM2;

namespace {
FILE* in;
template <class T>
std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, in) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}
template <class T>
T rd1() { return rd<T>(1)[0]; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]), 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    try {
        const int ncases = rd1<int32_t>();
        for (int c = 0; c < ncases; c++) {
            const int form = rd1<int32_t>(), nt = rd1<int32_t>();
            std::vector<KeyPoint> keys = rd<KeyPoint>(nt);
            std::vector<uint8_t> desc = rd<uint8_t>((size_t)nt * 32);
            std::vector<float> b = rd<float>(4);
            const int has_ur = rd1<int32_t>();
            std::vector<float> ur = rd<float>(has_ur ? nt : 0);
            std::vector<uint8_t> taken = rd<uint8_t>(nt);
            std::vector<float> scale = rd<float>(8);
            const float mbf = rd1<float>(), nnratio = rd1<float>();
            const int check_ori = rd1<int32_t>();
            const float th = rd1<float>();
            const int bMono = rd1<int32_t>(), fwd = rd1<int32_t>(), bwd = rd1<int32_t>(), nq = rd1<int32_t>();
            FrameGrid grid = form == 2 ? FrameGrid::Birdview(keys.data(), nt, 64.f / (b[1] - b[0]), 48.f / (b[3] - b[2]))
                                       : FrameGrid(keys.data(), nt, b[0], b[1], b[2], b[3]);
            FrameData F;
            F.n = nt;
            F.keys = keys.data();
            F.descriptors = desc.data();
            F.uRight = has_ur ? ur.data() : nullptr;
            F.hasMapPoint = taken.data();
            F.scaleFactors = scale.data();
            F.nlevels = 8;
            F.grid = &grid;
            ORBmatcher matcher(nnratio, check_ori != 0);
            std::vector<int> res;
            int n = 0;
            if (form == 0) {
                std::vector<float> u = rd<float>(nq), v = rd<float>(nq), iz = rd<float>(nq);
                std::vector<int32_t> oct = rd<int32_t>(nq);
                std::vector<float> ang = rd<float>(nq);
                std::vector<uint8_t> obs = rd<uint8_t>(nq), qd = rd<uint8_t>((size_t)nq * 32);
                ProjectedLastFrame L;
                L.bForward = fwd != 0;
                L.bBackward = bwd != 0;
                L.mbf = mbf;
                for (int i = 0; i < nq; i++)
                    L.points.push_back({u[i], v[i], iz[i], oct[i], ang[i], obs[i] != 0, &qd[(size_t)i * 32]});
                n = matcher.SearchByProjection(F, L, th, bMono != 0, res);
            } else if (form == 1) {
                std::vector<float> x = rd<float>(nq), y = rd<float>(nq), xr = rd<float>(nq);
                std::vector<int32_t> lv = rd<int32_t>(nq);
                std::vector<float> vc = rd<float>(nq);
                std::vector<uint8_t> qd = rd<uint8_t>((size_t)nq * 32);
                ProjectedMapPoints M;
                for (int i = 0; i < nq; i++) M.points.push_back({x[i], y[i], xr[i], lv[i], vc[i], &qd[(size_t)i * 32]});
                n = matcher.SearchByProjection(F, M, th, res);
            } else {
                std::vector<float> x = rd<float>(nq), y = rd<float>(nq);
                std::vector<uint8_t> qd = rd<uint8_t>((size_t)nq * 32);
                ProjectedBirdPoints B;
                for (int i = 0; i < nq; i++) B.points.push_back({x[i], y[i], &qd[(size_t)i * 32]});
                n = matcher.SearchByProjectionBird(F, B, th, res);
            }
            const int32_t head[2] = {n, (int32_t)res.size()};
            fwrite(head, 4, 2, out);
            if (!res.empty()) fwrite(res.data(), 4, res.size(), out);
        }
    } catch (const OrbGpuError& e) {
        fprintf(stderr, "OrbGpuError: %s\n", e.what());
        fclose(out);
        return 1;
    }
    fclose(out);
    return 0;
}
