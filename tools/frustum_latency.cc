// Per-call latency of the searches over resident map points against the staged path they replace, both through the
// C-ABI from one host thread:
//   frustum_latency <width> <height> <features> local <points> <reps>
//   frustum_latency <width> <height> <features> fuse <targets> <points per target> <reps>
// local: orb_search_local_points (ids up, k_project_points, k_projection_topk, the replay, records back) against a
//   single-thread loop with the same projection arithmetic (orb_project_points_host over the points' host arrays),
//   the staging of an orb_proj_query and a descriptor per visible point, and orb_search_by_projection_frame.
// fuse:  orb_fuse_search_points against the same loop per target, the staging, and orb_project_best_frames.
// The frame(s) are resident in both paths.  Seeded synthetic inputs: features uniform over the image on 8 levels, three
// quarters of the points back-projected from features (so the searches match), the others spread around the view.
// Warm-up calls, then <reps> timed ones of each path, alternating; medians.  One JSON object on stdout; exit status 1
// if the two paths disagree.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../include/orbgpu.h"

namespace {
typedef std::chrono::steady_clock Clock;
double us(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }
double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}
#define CHECK(call)                                                                     \
    do {                                                                                \
        const int st_ = (call);                                                         \
        if (st_ != ORB_OK) {                                                            \
            std::fprintf(stderr, "%s: %d (%s)\n", #call, st_, orb_last_error());        \
            std::exit(2);                                                               \
        }                                                                               \
    } while (0)

struct Scene {   // one camera with its frame and the points that look at it
    orb_camera cam;
    std::vector<orb_keypoint> kps;
    std::vector<uint8_t> desc;
    std::vector<float> uright, inv_sigma2;
    orb_frame* frame = nullptr;
    std::vector<float> pos, nrm, lo, hi;   // the points, in ids order
    std::vector<uint8_t> pdesc;
    std::vector<int> ids;
};

Scene make_scene(orb_ctx* ctx, std::mt19937& rng, int W, int H, int nfeat, int npoints, int slot0) {
    Scene S;
    std::uniform_real_distribution<float> U(0.f, 1.f);
    orb_camera& c = S.cam;
    std::memset(&c, 0, sizeof c);
    const float a = 0.05f + 0.1f * U(rng), ca = std::cos(a), sa = std::sin(a);   // a rotation about y
    const float R[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca};
    std::memcpy(c.Rcw, R, sizeof R);
    c.tcw[0] = 0.3f * U(rng);
    c.tcw[1] = -0.2f * U(rng);
    c.tcw[2] = 0.5f * U(rng);
    for (int i = 0; i < 3; i++) c.Ow[i] = -(R[i] * c.tcw[0] + R[3 + i] * c.tcw[1] + R[6 + i] * c.tcw[2]);
    c.fx = c.fy = 0.8f * W;
    c.cx = 0.5f * W;
    c.cy = 0.5f * H;
    c.mbf = 40.f;
    c.min_x = c.min_y = 0.f;
    c.max_x = (float)W;
    c.max_y = (float)H;
    c.nlevels = 8;
    c.log_scale_factor = std::log(1.2f);
    S.inv_sigma2.resize(8);
    float s = 1.f;
    for (int l = 0; l < 8; l++, s *= 1.2f) {
        c.scale_factors[l] = s;
        S.inv_sigma2[l] = 1.f / (s * s);
    }
    S.kps.resize(nfeat);
    S.desc.resize((size_t)nfeat * 32);
    S.uright.resize(nfeat);
    for (int i = 0; i < nfeat; i++) {
        orb_keypoint& k = S.kps[i];
        std::memset(&k, 0, sizeof k);
        k.x = 2.f + (W - 4.f) * U(rng);
        k.y = 2.f + (H - 4.f) * U(rng);
        k.octave = (int)(rng() % 8);
        k.angle = 360.f * U(rng);
        S.uright[i] = i % 3 == 0 ? k.x - (0.5f + 3.5f * U(rng)) : -1.f;
        for (int b = 0; b < 32; b++) S.desc[(size_t)i * 32 + b] = (uint8_t)rng();
    }
    CHECK(orb_frame_create(ctx, nfeat, S.desc.data(), S.kps.data(), S.uright.data(), 0.f, 0.f, 64.f / W, 48.f / H,
                           &S.frame));
    S.pos.resize(3 * (size_t)npoints);
    S.nrm.resize(3 * (size_t)npoints);
    S.lo.resize(npoints);
    S.hi.resize(npoints);
    S.pdesc.resize((size_t)npoints * 32);
    S.ids.resize(npoints);
    for (int i = 0; i < npoints; i++) {
        S.ids[i] = slot0 + i;
        const bool on_feature = rng() % 4 != 0;
        const int f = (int)(rng() % nfeat);
        float u = S.kps[f].x, v = S.kps[f].y, z = 2.f + 7.f * U(rng);
        if (!on_feature) {
            u = -0.25f * W + 1.5f * W * U(rng);
            v = -0.25f * H + 1.5f * H * U(rng);
            if (rng() % 5 == 0) z = -z;
        }
        const float Pc[3] = {(u - c.cx) / c.fx * z - c.tcw[0], (v - c.cy) / c.fy * z - c.tcw[1], z - c.tcw[2]};
        float PO[3], d = 0;
        for (int k = 0; k < 3; k++) {
            S.pos[3 * (size_t)i + k] = R[k] * Pc[0] + R[3 + k] * Pc[1] + R[6 + k] * Pc[2];   // R^T (Pc - t)
            PO[k] = S.pos[3 * (size_t)i + k] - c.Ow[k];
            d += PO[k] * PO[k];
        }
        d = std::sqrt(d);
        for (int k = 0; k < 3; k++)
            S.nrm[3 * (size_t)i + k] = (on_feature ? 1.f : (U(rng) < 0.5f ? 1.f : -1.f)) * PO[k] / d;
        S.lo[i] = d * (on_feature ? 0.5f : 0.4f + 1.1f * U(rng));
        S.hi[i] = d * std::pow(1.2f, (float)S.kps[f].octave - 0.5f);
        std::memcpy(&S.pdesc[(size_t)i * 32], &S.desc[(size_t)f * 32], 32);
        if (on_feature)
            for (int b = (int)(rng() % 7); b > 0; b--) S.pdesc[(size_t)i * 32 + rng() % 32] ^= (uint8_t)(1u << (rng() % 8));
        else
            for (int b = 0; b < 32; b++) S.pdesc[(size_t)i * 32 + b] = (uint8_t)rng();
    }
    return S;
}

// The staged path's host step for one scene: the projection loop, then a query and a descriptor per visible point
int stage(const Scene& S, int mode, float th, std::vector<orb_point_proj>& rec, std::vector<orb_proj_query>& q,
          std::vector<uint8_t>& qd, std::vector<int>& where) {
    const int n = (int)S.ids.size();
    rec.resize(n);
    CHECK(orb_project_points_host(mode, &S.cam, 0.5f, th, n, S.pos.data(), S.nrm.data(), S.lo.data(), S.hi.data(),
                                  rec.data()));
    q.clear();
    qd.resize((size_t)n * 32);
    where.clear();
    for (int i = 0; i < n; i++) {
        const orb_point_proj& p = rec[i];
        if (p.verdict != ORB_POINT_VISIBLE) continue;
        std::memcpy(&qd[q.size() * 32], &S.pdesc[(size_t)i * 32], 32);
        q.push_back(orb_proj_query{p.u, p.v, p.r, p.level - 1, p.level, p.ur, mode == ORB_FRUSTUM_FRAME ? p.r : 0.f, 0.f, 1});
        where.push_back(i);
    }
    return (int)q.size();
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 7) return std::fprintf(stderr, "usage: %s W H features local|fuse ... reps\n", argv[0]), 2;
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), nfeat = std::atoi(argv[3]);
    const bool fuse = !std::strcmp(argv[4], "fuse");
    const int ntargets = fuse ? std::atoi(argv[5]) : 1, npoints = std::atoi(argv[fuse ? 6 : 5]);
    const int reps = std::atoi(argv[fuse ? 7 : 6]), warmup = 30;
    orb_params p;
    std::memset(&p, 0, sizeof p);
    p.nfeatures = 1000;
    p.scaleFactor = 1.2f;
    p.nlevels = 8;
    p.iniThFAST = 20;
    p.minThFAST = 7;
    int st = 0;
    orb_ctx* ctx = orb_create(&p, &st);
    if (!ctx) return std::fprintf(stderr, "orb_create: %d (%s)\n", st, orb_last_error()), 2;
    std::mt19937 rng(20241020);
    std::vector<Scene> scenes;
    orb_points* P = nullptr;
    CHECK(orb_points_create(ctx, ntargets * npoints, &P));
    for (int t = 0; t < ntargets; t++) {
        scenes.push_back(make_scene(ctx, rng, W, H, nfeat, npoints, t * npoints));
        const Scene& S = scenes.back();
        CHECK(orb_points_write(P, t * npoints, npoints, S.pos.data(), S.nrm.data(), S.lo.data(), S.hi.data(),
                               S.pdesc.data()));
    }
    const float th = fuse ? 3.0f : 1.0f, nnratio = 0.8f;
    std::vector<double> t_new, t_old, t_loop;
    long visible = 0, found_new = 0, found_old = 0;
    bool equal = true;
    if (!fuse) {
        const Scene& S = scenes[0];
        std::vector<int> m_new(nfeat), m_old(nfeat), where;
        std::vector<orb_point_proj> rec_new(npoints), rec_old;
        std::vector<orb_proj_query> q;
        std::vector<uint8_t> qd;
        for (int r = 0; r < warmup + reps; r++) {
            int nm_new = 0, nm_old = 0;
            const Clock::time_point a = Clock::now();
            CHECK(orb_search_local_points(ctx, P, &S.cam, 0.5f, th, nnratio, npoints, S.ids.data(), S.frame, nullptr, 1,
                                          m_new.data(), &nm_new, rec_new.data()));
            const Clock::time_point b = Clock::now();
            const int nvis = stage(S, ORB_FRUSTUM_FRAME, th, rec_old, q, qd, where);
            const Clock::time_point c = Clock::now();
            CHECK(orb_search_by_projection_frame(ctx, ORB_PROJ_RATIO_SAME_LEVEL, nnratio, 0, 100, nvis, q.data(),
                                                 qd.data(), S.frame, nullptr, 1, m_old.data(), &nm_old));
            const Clock::time_point d = Clock::now();
            if (r >= warmup) {
                t_new.push_back(us(a, b));
                t_old.push_back(us(b, d));
                t_loop.push_back(us(b, c));
            }
            for (int& m : m_old)
                if (m >= 0) m = where[m];
            equal = equal && nm_new == nm_old && m_new == m_old &&
                    !std::memcmp(rec_new.data(), rec_old.data(), (size_t)npoints * sizeof(orb_point_proj));
            visible = nvis;
            found_new = nm_new;
            found_old = nm_old;
        }
    } else {
        std::vector<orb_fuse_points_target> T(ntargets);
        std::vector<orb_proj_frame_target> F(ntargets);
        std::vector<std::vector<int> > bi(ntargets), bd(ntargets), si(ntargets), sd(ntargets), where(ntargets);
        std::vector<std::vector<orb_point_proj> > rec_new(ntargets), rec_old(ntargets);
        std::vector<std::vector<orb_proj_query> > q(ntargets);
        std::vector<std::vector<uint8_t> > qd(ntargets);
        for (int t = 0; t < ntargets; t++) {
            const Scene& S = scenes[t];
            bi[t].resize(npoints);
            bd[t].resize(npoints);
            si[t].resize(npoints);
            sd[t].resize(npoints);
            rec_new[t].resize(npoints);
            T[t] = orb_fuse_points_target{S.cam, S.frame, S.inv_sigma2.data(), th, npoints, S.ids.data(), bi[t].data(),
                                          bd[t].data(), rec_new[t].data()};
        }
        for (int r = 0; r < warmup + reps; r++) {
            const Clock::time_point a = Clock::now();
            CHECK(orb_fuse_search_points(ctx, P, ntargets, T.data()));
            const Clock::time_point b = Clock::now();
            for (int t = 0; t < ntargets; t++) {
                const int nvis = stage(scenes[t], ORB_FRUSTUM_FUSE, th, rec_old[t], q[t], qd[t], where[t]);
                F[t] = orb_proj_frame_target{nvis, q[t].data(), qd[t].data(), scenes[t].frame,
                                             scenes[t].inv_sigma2.data(), 8, si[t].data(), sd[t].data()};
            }
            const Clock::time_point c = Clock::now();
            CHECK(orb_project_best_frames(ctx, ORB_PROJ_GATE_FUSE, ntargets, F.data()));
            const Clock::time_point d = Clock::now();
            if (r >= warmup) {
                t_new.push_back(us(a, b));
                t_old.push_back(us(b, d));
                t_loop.push_back(us(b, c));
            }
            visible = found_new = found_old = 0;
            for (int t = 0; t < ntargets; t++) {
                visible += (long)where[t].size();
                std::vector<int> full(npoints, -1), fulld(npoints, -1);
                for (size_t k = 0; k < where[t].size(); k++) {
                    full[where[t][k]] = si[t][k];
                    fulld[where[t][k]] = sd[t][k];
                    found_old += si[t][k] >= 0;
                }
                for (int i = 0; i < npoints; i++) found_new += bi[t][i] >= 0;
                equal = equal && full == bi[t] && fulld == bd[t] &&
                        !std::memcmp(rec_new[t].data(), rec_old[t].data(), (size_t)npoints * sizeof(orb_point_proj));
            }
        }
    }
    std::printf("{\"call\": \"%s\", \"width\": %d, \"height\": %d, \"features\": %d, \"targets\": %d, \"points\": %d, "
                "\"visible\": %ld, \"found\": %ld, \"found_staged\": %ld, \"equal\": %s, \"reps\": %d, "
                "\"resident_us_median\": %.1f, \"staged_us_median\": %.1f, \"staged_host_loop_us_median\": %.1f, "
                "\"staged_over_resident\": %.3f}\n",
                fuse ? "orb_fuse_search_points" : "orb_search_local_points", W, H, nfeat, ntargets, npoints, visible,
                found_new, found_old, equal ? "true" : "false", reps, median(t_new), median(t_old), median(t_loop),
                median(t_old) / median(t_new));
    for (Scene& S : scenes) orb_frame_destroy(S.frame);
    orb_points_destroy(P);
    orb_destroy(ctx);
    return equal ? 0 : 1;
}
