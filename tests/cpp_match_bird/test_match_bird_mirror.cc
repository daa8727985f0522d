// Drives the host mirror's SearchByMatchBird the way Tracking drives the reference's:
//   test_match_bird_mirror <cases.bin> <results.bin>
// cases.bin (little endian, written by tests/test_gpu_match_bird_mirror.py): int32 ncases, then per case
//   int32 form (0: SearchByMatchBird(KeyFrame*, Frame&, ...), 1: SearchByMatchBird(CurrentFrame, LastFrame, ...))
//   the Frame (form 1: CurrentFrame): int32 nt | nt keypoints (28 B) | nt descriptors (32 B) | float bounds[4]
//   float nnratio | int32 check_ori | float r (form 1: windowSize)
//   form 0: int32 nq | nq int32 index | nq float x, y, angle | nq descriptors
//   form 1: int32 n_last | n_last keypoints | n_last descriptors | int32 has_mp | n_last uint8 (if has_mp)
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
            const float nnratio = rd1<float>();
            const int check_ori = rd1<int32_t>();
            const float r = rd1<float>();
            FrameGrid grid = FrameGrid::Birdview(keys.data(), nt, 64.f / (b[1] - b[0]), 48.f / (b[3] - b[2]));
            FrameData F;
            F.n = nt;
            F.keys = keys.data();
            F.descriptors = desc.data();
            F.grid = &grid;
            ORBmatcher matcher(nnratio, check_ori != 0);
            std::vector<int> res;
            int n = 0;
            if (form == 0) {
                const int nq = rd1<int32_t>();
                std::vector<int32_t> id = rd<int32_t>(nq);
                std::vector<float> x = rd<float>(nq), y = rd<float>(nq), ang = rd<float>(nq);
                std::vector<uint8_t> qd = rd<uint8_t>((size_t)nq * 32);
                KeyFrameBirdPoints KF;
                for (int i = 0; i < nq; i++) KF.points.push_back({id[i], x[i], y[i], ang[i], &qd[(size_t)i * 32]});
                n = matcher.SearchByMatchBird(KF, F, res, r);
            } else {
                const int nl = rd1<int32_t>();
                std::vector<KeyPoint> lkeys = rd<KeyPoint>(nl);
                std::vector<uint8_t> ldesc = rd<uint8_t>((size_t)nl * 32);
                const int has_mp = rd1<int32_t>();
                std::vector<uint8_t> mp = rd<uint8_t>(has_mp ? nl : 0);
                FrameData L;
                L.n = nl;
                L.keys = lkeys.data();
                L.descriptors = ldesc.data();
                L.hasMapPoint = has_mp ? mp.data() : nullptr;
                n = matcher.SearchByMatchBird(F, L, (int)r, res);
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
