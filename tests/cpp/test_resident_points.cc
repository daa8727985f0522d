// Runs the host mirror's searches over ResidentPoints next to the staged mirror calls fed with the records' visible
// points:
//   test_resident_points <cases.bin> <results.bin>
// cases.bin (little endian, written by tests/test_gpu_resident_points_mirror.py):
//   int32 nslots | 3 nslots float pos | 3 nslots float normal | nslots float min_dist | nslots float max_dist |
//     nslots descriptors
//   the SearchLocalPoints case: orb_camera | float th, view_cos_limit, nnratio | int32 nids | ids | a frame
//   the FuseSearch case: int32 ntargets | per target: orb_camera | float th | int32 nids | ids | a frame |
//     camera.nlevels float inv_sigma2
//   a frame: int32 nt | nt keypoints | nt descriptors | float bounds[4] | int32 has_ur | nt float uright (if has_ur) |
//     nt bytes taken
// results.bin: SearchLocalPoints: int32 nmatches (resident), nmatches (staged), nt, nids | nt int32 (resident) | nt int32
//   (staged, as positions in ids) | nids orb_point_proj; FuseSearch: per target int32 n | n (idx, dist) int32 pairs
//   (resident, all targets in one call) | the same (staged) | n orb_point_proj.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <utility>
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

struct FrameCase {
    int nt = 0, has_ur = 0;
    std::vector<KeyPoint> keys;
    std::vector<uint8_t> desc, taken;
    std::vector<float> b, ur;
    void read() {
        nt = rd1<int32_t>();
        keys = rd<KeyPoint>(nt);
        desc = rd<uint8_t>((size_t)nt * 32);
        b = rd<float>(4);
        has_ur = rd1<int32_t>();
        ur = rd<float>(has_ur ? nt : 0);
        taken = rd<uint8_t>(nt);
    }
    ResidentFrame resident() const {
        return ResidentFrame(keys.data(), nt, desc.data(), has_ur ? ur.data() : nullptr, b[0], b[1], b[2], b[3]);
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]), 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    try {
        const int nslots = rd1<int32_t>();
        std::vector<float> pos = rd<float>(3 * (size_t)nslots), nrm = rd<float>(3 * (size_t)nslots),
                           lo = rd<float>(nslots), hi = rd<float>(nslots);
        std::vector<uint8_t> pdesc = rd<uint8_t>((size_t)nslots * 32);
        // written in two ranges into a handle that starts too small (it grows), then moved once (move-only)
        ResidentPoints made(8);
        const int half = nslots / 2;
        made.Write(0, half, pos.data(), nrm.data(), lo.data(), hi.data(), pdesc.data());
        made.Write(half, nslots - half, &pos[3 * (size_t)half], &nrm[3 * (size_t)half], &lo[half], &hi[half],
                   &pdesc[(size_t)half * 32]);
        ResidentPoints P(std::move(made));
        if (made || !P || P.Capacity() < nslots) return fprintf(stderr, "ResidentPoints move / growth\n"), 1;
        {   // SearchLocalPoints against SearchByProjection(ResidentFrame, members, ProjectedMapPoints, th)
            const orb_camera cam = rd1<orb_camera>();
            const float th = rd1<float>(), limit = rd1<float>(), nnratio = rd1<float>();
            const int nids = rd1<int32_t>();
            std::vector<int> ids = rd<int32_t>(nids);
            FrameCase fc;
            fc.read();
            ResidentFrame R = fc.resident();
            FrameData members;
            members.hasMapPoint = fc.taken.data();
            members.scaleFactors = cam.scale_factors;
            members.nlevels = cam.nlevels;
            ORBmatcher matcher(nnratio, true);
            std::vector<int> res, staged;
            std::vector<orb_point_proj> proj;
            const int n_res = matcher.SearchLocalPoints(P, cam, ids, R, members, th, limit, res, &proj);
            ProjectedMapPoints M;
            std::vector<int> where;   // the position in ids of each visible point
            for (int i = 0; i < nids; i++)
                if (proj[i].verdict == ORB_POINT_VISIBLE) {
                    M.points.push_back({proj[i].u, proj[i].v, proj[i].ur, proj[i].level, proj[i].view_cos,
                                        &pdesc[(size_t)ids[i] * 32]});
                    where.push_back(i);
                }
            const int n_st = matcher.SearchByProjection(R, members, M, th, staged);
            for (int& m : staged)
                if (m >= 0) m = where[m];
            // without the records the matches are the same
            std::vector<int> res2;
            if (matcher.SearchLocalPoints(P, cam, ids, R, members, th, limit, res2) != n_res || res2 != res)
                return fprintf(stderr, "SearchLocalPoints without records differs\n"), 1;
            const int32_t head[4] = {n_res, n_st, fc.nt, nids};
            fwrite(head, 4, 4, out);
            fwrite(res.data(), 4, res.size(), out);
            fwrite(staged.data(), 4, staged.size(), out);
            fwrite(proj.data(), sizeof(orb_point_proj), proj.size(), out);
        }
        {   // FuseSearch(ResidentPoints, ...) against FuseSearch(targets with kf.resident, chi2Gate = true)
            const int ntargets = rd1<int32_t>();
            std::vector<FusePointsTarget> T(ntargets);
            std::vector<FuseTarget> S(ntargets);
            std::vector<ResidentFrame> frames(ntargets);
            std::vector<std::vector<float> > inv(ntargets);
            std::vector<FrameCase> fcs(ntargets);
            for (int t = 0; t < ntargets; t++) {
                T[t].camera = rd1<orb_camera>();
                T[t].th = rd1<float>();
                T[t].ids = rd<int32_t>(rd1<int32_t>());
                fcs[t].read();
                inv[t] = rd<float>(T[t].camera.nlevels);
                frames[t] = fcs[t].resident();
                T[t].kf = &frames[t];
                T[t].invLevelSigma2 = inv[t].data();
            }
            ORBmatcher matcher(0.6f, true);
            std::vector<std::vector<FuseBest> > best, staged;
            std::vector<std::vector<orb_point_proj> > proj;
            matcher.FuseSearch(P, T, best, &proj);
            std::vector<std::vector<int> > where(ntargets);
            for (int t = 0; t < ntargets; t++) {
                S[t].kf.n = fcs[t].nt;
                S[t].kf.invLevelSigma2 = inv[t].data();
                S[t].kf.nlevels = T[t].camera.nlevels;
                S[t].kf.resident = &frames[t];
                for (size_t i = 0; i < T[t].ids.size(); i++) {
                    const orb_point_proj& p = proj[t][i];
                    if (p.verdict != ORB_POINT_VISIBLE) continue;
                    S[t].points.push_back({p.u, p.v, p.ur, p.level, p.r, &pdesc[(size_t)T[t].ids[i] * 32]});
                    where[t].push_back((int)i);
                }
            }
            matcher.FuseSearch(S, true, staged);
            for (int t = 0; t < ntargets; t++) {
                const int32_t n = (int32_t)T[t].ids.size();
                std::vector<FuseBest> full(n, FuseBest{-1, -1});
                for (size_t k = 0; k < where[t].size(); k++) full[where[t][k]] = staged[t][k];
                fwrite(&n, 4, 1, out);
                fwrite(best[t].data(), sizeof(FuseBest), n, out);
                fwrite(full.data(), sizeof(FuseBest), n, out);
                fwrite(proj[t].data(), sizeof(orb_point_proj), n, out);
            }
        }
        // failures throw OrbGpuError: a search on a moved-from handle, and a slot outside the capacity
        int threw = 0;
        try {
            std::vector<std::vector<FuseBest> > b;
            ORBmatcher(0.6f, true).FuseSearch(made, std::vector<FusePointsTarget>(), b);
        } catch (const OrbGpuError&) {
            threw++;
        }
        try {
            made.Write(0, 1, pos.data(), nrm.data(), lo.data(), hi.data(), pdesc.data());
        } catch (const OrbGpuError&) {
            threw++;
        }
        if (threw != 2) return fprintf(stderr, "an empty ResidentPoints was accepted\n"), 1;
    } catch (const OrbGpuError& e) {
        fprintf(stderr, "OrbGpuError: %s\n", e.what());
        fclose(out);
        return 1;
    }
    fclose(out);
    return 0;
}
