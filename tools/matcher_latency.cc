// Per-call latency of the ORBmatcher drop-ins at the reference's call granularity (bench.py `matcher`
// leg): one call per frame / keyframe pair, as Tracking / LocalMapping / LoopClosing make them.
//
//   SearchByBoW(KeyFrame*, Frame&)       ORBmatcher(0.7, true)   Tracking::TrackReferenceKeyFrame, Tracking.cc:1029-1032
//   SearchByBoW(KeyFrame*, KeyFrame*)    ORBmatcher(0.75, true)  LoopClosing::ComputeSim3, LoopClosing.cc:265
//   SearchForTriangulation               ORBmatcher(0.6, false)  LocalMapping::CreateNewMapPoints, LocalMapping.cc:225,278
//   SearchForInitialization (window 100) ORBmatcher(0.9, true)   Tracking::MonocularInitialization, Tracking.cc:738-739
//   Frame::ComputeBoW (transform, levelsup 4)                    Frame.cc:562-569
//   Frame::ComputeStereoMatches (rectified pair, KITTI mb / mbf)  Frame.cc:662-836, from the stereo Frame ctor :141
//     (only when frames.raw holds four frames: the last two are the left / right images)
//
// GPU side: the reference-signature adapter (adapter/ORBmatcher_gpu.cc) on Frame / KeyFrame objects
// (tests/cpp/slam_api models; their grid lookups are the caller's CPU code, Frame.cc:378-547), and the
// host-mirror ORBVocabulary.  Features: the GPU ORBextractor on two C3 frames (the second a shifted
// copy of the first), FeatureVectors from the GPU vocabulary transform of a synthetic k = 10, L = 6
// vocabulary in ORBvoc.bin's format.  CPU side (the baseline, single thread): the oracle's restatement
// of each reference body (oracle/orb_oracle.cpp) on the same inputs -- for SearchForInitialization
// including the per-keypoint GetFeaturesInArea queries on the frame's grid, as the reference loop
// makes them.  Every GPU output is checked equal to the oracle's before anything is timed.
//
//   SearchByMatchBird (both forms)       ORBmatcher(0.99, true)  Tracking::TrackReferenceKeyFrame, Tracking.cc:1046 (r = 15), and
//     TrackWithMotionModel, :1241 (window 15): only with a trailing `bird` argument, on the two frames' features
//     standing for the birdview stream's (run it at 1280x720 / 2000 features, the stream's size); GPU = the C-ABI
//     calls the host mirror makes (orb_search_by_match_bird, orb_search_by_match_bird_frame), CPU = the reference
//     loops (ORBmatcher.cc:1790-1921, :2000-2114) written out below over the Frame's own grid, single thread.
//
// usage: matcher_latency <frames.raw> <w> <h> <nfeatures> <vocab.bin> <reps> [cpu_reps [bird]]
// Prints one JSON line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <utility>
#include <vector>

#include "../oracle/orb_oracle.h"
#include "../orb-slam-birdview_amd/host/ORBVocabulary.h"
#include "../orb-slam-birdview_amd/host/ORBextractor.h"
#include "../orb-slam-birdview_amd/host/Stereo.h"
#include "../include/orbgpu.h"
#include "ORBmatcher.h"   // tests/cpp/slam_api: the reference's declaration, modelled

using namespace ORB_SLAM2;

template <class F>
static double median_us(F f, int reps) {
    f();   // warm: context creation, scratch growth
    std::vector<double> t;
    for (int i = 0; i < reps; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

struct Feat {
    std::vector<cv::KeyPoint> kps;
    cv::Mat desc;
    DBoW2::FeatureVector fv;
};

struct OFv {   // oracle CSR of a FeatureVector
    std::vector<uint32_t> ids;
    std::vector<int> off, idx;
    OracleFeatVec fv;
    explicit OFv(const DBoW2::FeatureVector& f) {
        off.push_back(0);
        for (auto it = f.begin(); it != f.end(); ++it) {
            ids.push_back(it->first);
            for (unsigned v : it->second) idx.push_back((int)v);
            off.push_back((int)idx.size());
        }
        if (idx.empty()) idx.push_back(0);
        fv.nnodes = (int)ids.size();
        fv.node_ids = ids.data();
        fv.offsets = off.data();
        fv.indices = idx.data();
    }
};

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static std::vector<float> angles(const std::vector<cv::KeyPoint>& k) {
    std::vector<float> a(k.size() + 1, 0.f);
    for (size_t i = 0; i < k.size(); i++) a[i] = k[i].angle;
    return a;
}

int main(int argc, char** argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s frames.raw w h nfeatures vocab.bin reps [cpu_reps]\n", argv[0]);
        return 2;
    }
    const int w = atoi(argv[2]), h = atoi(argv[3]), nfeat = atoi(argv[4]), reps = atoi(argv[6]);
    const int cpu_reps = argc > 7 ? atoi(argv[7]) : std::max(3, reps / 5);
    std::vector<uint8_t> frames((size_t)w * h * 4);
    FILE* fp = fopen(argv[1], "rb");
    const size_t nread = fp ? fread(frames.data(), 1, frames.size(), fp) : 0;
    if (!fp || (nread != frames.size() / 2 && nread != frames.size())) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(fp);
    const bool with_stereo = nread == frames.size();

    // ---- features: GPU extractor + GPU vocabulary (the product)
    ORBextractor ex(nfeat, 1.2f, 8, 20, 7, 0);
    ORBVocabulary voc(0);
    if (!voc.loadFromBinaryFile(argv[5])) {
        fprintf(stderr, "cannot load %s\n", argv[5]);
        return 2;
    }
    Feat fe[2];
    std::vector<ORB_SLAM2::KeyPoint> hk;
    DescriptorMat hd;
    DescriptorMat descs[2];
    for (int f = 0; f < 2; f++) {
        ex(ImageView(frames.data() + (size_t)f * w * h, w, h), ImageView(), hk, hd);
        fe[f].kps.resize(hk.size());
        memcpy((void*)fe[f].kps.data(), hk.data(), hk.size() * sizeof(orb_keypoint));
        fe[f].desc = cv::Mat((int)hk.size(), 32, CV_8U);
        memcpy(fe[f].desc.data, hd.buf.data(), hk.size() * 32);
        descs[f] = hd;
        BowVector bv;
        BowFeatureVector bfv;
        voc.transform(hd, bv, bfv, 4);
        for (auto& kv : bfv) fe[f].fv[kv.first] = kv.second;
    }
    const int nA = (int)fe[0].kps.size(), nB = (int)fe[1].kps.size();
    std::vector<float> scale(8), sigma2(8);
    {
        std::vector<float> s = ex.GetScaleFactors(), s2 = ex.GetScaleSigmaSquares();
        for (int l = 0; l < 8; l++) scale[l] = s[l], sigma2[l] = s2[l];
    }

    // ---- the SLAM objects (as make_kf in tests/cpp/test_matcher_adapter.cc)
    std::vector<MapPoint*> pool;
    KeyFrame KF[2];
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const float tw[2][3] = {{0, 0, 0}, {-0.35f, 0.f, 0.02f}};
    for (int f = 0; f < 2; f++) {
        KeyFrame& kf = KF[f];
        kf.N = (int)fe[f].kps.size();
        kf.mvKeysUn = fe[f].kps;
        kf.mDescriptors = fe[f].desc;
        kf.mFeatVec = fe[f].fv;
        kf.mvScaleFactors = scale;
        kf.mvLevelSigma2 = sigma2;
        kf.fx = kf.fy = 700.f;
        kf.cx = w * 0.5f;
        kf.cy = h * 0.5f;
        kf.SetPose(I, tw[f]);
        kf.mvpMapPoints.assign(kf.N, nullptr);
        kf.mvuRight.assign(kf.N, -1.f);
        uint32_t s = 11u + 18u * f;
        for (int i = 0; i < kf.N; i++) {
            if (lcg(s) % 10 < 7) {
                pool.push_back(new MapPoint(lcg(s) % 10 == 0));
                kf.mvpMapPoints[i] = pool.back();
            }
            if (lcg(s) % 10 < 3) kf.mvuRight[i] = fe[f].kps[i].pt.x - 5.f;
        }
    }
    Frame F[2];
    for (int f = 0; f < 2; f++) {
        F[f].N = (int)fe[f].kps.size();
        F[f].mvKeys = F[f].mvKeysUn = fe[f].kps;
        F[f].mDescriptors = fe[f].desc;
        F[f].mFeatVec = fe[f].fv;
        F[f].mnMinX = 0;
        F[f].mnMaxX = (float)w;
        F[f].mnMinY = 0;
        F[f].mnMaxY = (float)h;
        F[f].AssignFeaturesToGrid();   // Frame constructor (Frame.cc:141)
    }
    const std::vector<float> aA = angles(fe[0].kps), aB = angles(fe[1].kps);
    const OFv fvA(fe[0].fv), fvB(fe[1].fv);
    std::vector<uint8_t> mpA(nA + 1, 0), mpB(nB + 1, 0);
    for (int i = 0; i < nA; i++) mpA[i] = KF[0].mvpMapPoints[i] && !KF[0].mvpMapPoints[i]->isBad();
    for (int i = 0; i < nB; i++) mpB[i] = KF[1].mvpMapPoints[i] && !KF[1].mvpMapPoints[i]->isBad();
    const OracleKeyPoint* okA = reinterpret_cast<const OracleKeyPoint*>(fe[0].kps.data());
    const OracleKeyPoint* okB = reinterpret_cast<const OracleKeyPoint*>(fe[1].kps.data());

    std::string out = "{";
    bool all_ok = true;
    char buf[512];
    auto emit = [&](const char* name, double gpu, double cpu, int nm, int onm, bool ok) {
        all_ok = all_ok && ok;
        snprintf(buf, sizeof buf, "%s\"%s\": {\"gpu_us\": %.1f, \"cpu_us\": %.1f, \"speedup\": %.2f, \"matches\": %d, "
                 "\"oracle_matches\": %d, \"equal\": %s}", out.size() > 1 ? ", " : "", name, gpu, cpu, cpu / gpu, nm, onm,
                 ok ? "true" : "false");
        out += buf;
    };

    // ---- SearchByBoW(KF, F)
    {
        ORBmatcher m(0.7f, true);
        std::vector<MapPoint*> v;
        const int nm = m.SearchByBoW(&KF[0], F[1], v);
        std::vector<int> om(nB + 1, -1);
        const int onm = oracle_search_by_bow_kf_f(0.7f, 1, nA, fe[0].desc.data, aA.data(), mpA.data(), fvA.fv, nB,
                                                  fe[1].desc.data, aB.data(), fvB.fv, om.data());
        bool ok = nm == onm && (int)v.size() == nB;
        for (int i = 0; ok && i < nB; i++) ok = v[i] == (om[i] >= 0 ? KF[0].mvpMapPoints[om[i]] : nullptr);
        const double g = median_us([&] { m.SearchByBoW(&KF[0], F[1], v); }, reps);
        const double c = median_us([&] {
            oracle_search_by_bow_kf_f(0.7f, 1, nA, fe[0].desc.data, aA.data(), mpA.data(), fvA.fv, nB, fe[1].desc.data,
                                      aB.data(), fvB.fv, om.data());
        }, cpu_reps);
        emit("SearchByBoW_KF_F", g, c, nm, onm, ok);
        // Tracking::Relocalization's candidate loop (Tracking.cc:1931-1938) as one batched call: 10 keyframes (the
        // same one: the same work per entry) against 10 runs of the CPU loop
        std::vector<KeyFrame*> vk(10, &KF[0]);
        std::vector<std::vector<MapPoint*> > vv;
        std::vector<int> vn;
        const int tot = m.SearchByBoW(vk, F[1], vv, vn);
        bool bok = tot == 10 * onm && (int)vv.size() == 10;
        for (int p = 0; bok && p < 10; p++) bok = vv[p] == v;
        const double gb = median_us([&] { m.SearchByBoW(vk, F[1], vv, vn); }, reps);
        emit("SearchByBoW_KF_F_x10", gb, 10 * c, tot, 10 * onm, bok && ok);
    }
    // ---- SearchByBoW(KF, KF)
    {
        ORBmatcher m(0.75f, true);
        std::vector<MapPoint*> v;
        const int nm = m.SearchByBoW(&KF[0], &KF[1], v);
        std::vector<int> om(nA + 1, -1);
        const int onm = oracle_search_by_bow_kf_kf(0.75f, 1, nA, fe[0].desc.data, aA.data(), mpA.data(), fvA.fv, nB,
                                                   fe[1].desc.data, aB.data(), mpB.data(), fvB.fv, om.data());
        bool ok = nm == onm && (int)v.size() == nA;
        for (int i = 0; ok && i < nA; i++) ok = v[i] == (om[i] >= 0 ? KF[1].mvpMapPoints[om[i]] : nullptr);
        const double g = median_us([&] { m.SearchByBoW(&KF[0], &KF[1], v); }, reps);
        const double c = median_us([&] {
            oracle_search_by_bow_kf_kf(0.75f, 1, nA, fe[0].desc.data, aA.data(), mpA.data(), fvA.fv, nB,
                                       fe[1].desc.data, aB.data(), mpB.data(), fvB.fv, om.data());
        }, cpu_reps);
        emit("SearchByBoW_KF_KF", g, c, nm, onm, ok);
        // LoopClosing::ComputeSim3's candidate loop (LoopClosing.cc:252-265) as one batched call: 10 candidates
        std::vector<KeyFrame*> vk(10, &KF[1]);
        std::vector<std::vector<MapPoint*> > vv;
        std::vector<int> vn;
        const int tot = m.SearchByBoW(&KF[0], vk, vv, vn);
        bool bok = tot == 10 * onm && (int)vv.size() == 10;
        for (int p = 0; bok && p < 10; p++) bok = vv[p] == v;
        const double gb = median_us([&] { m.SearchByBoW(&KF[0], vk, vv, vn); }, reps);
        emit("SearchByBoW_KF_KF_x10", gb, 10 * c, tot, 10 * onm, bok && ok);
    }
    // ---- SearchForTriangulation (R = I, F12 = K^-T [t12]x K^-1, LocalMapping::ComputeF12's form)
    {
        const double t12[3] = {tw[0][0] - tw[1][0], tw[0][1] - tw[1][1], tw[0][2] - tw[1][2]};
        const double fx = 700, cx = w * 0.5, cy = h * 0.5;
        const double Kinv[3][3] = {{1 / fx, 0, -cx / fx}, {0, 1 / fx, -cy / fx}, {0, 0, 1}};
        const double tx[3][3] = {{0, -t12[2], t12[1]}, {t12[2], 0, -t12[0]}, {-t12[1], t12[0], 0}};
        double M[3][3], Fd[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                M[i][j] = 0;
                for (int k = 0; k < 3; k++) M[i][j] += tx[i][k] * Kinv[k][j];
            }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                Fd[i][j] = 0;
                for (int k = 0; k < 3; k++) Fd[i][j] += Kinv[k][i] * M[k][j];
            }
        cv::Mat F12(3, 3, CV_32F);
        float Fv[9];
        for (int i = 0; i < 9; i++) Fv[i] = F12.at<float>(i / 3, i % 3) = (float)Fd[i / 3][i % 3];
        ORBmatcher m(0.6f, false);
        std::vector<std::pair<size_t, size_t> > v;
        const int nm = m.SearchForTriangulation(&KF[0], &KF[1], F12, v, false);
        cv::Mat Cw = KF[0].GetCameraCenter(), R2w = KF[1].GetRotation(), t2w = KF[1].GetTranslation();
        cv::Mat C2 = R2w * Cw + t2w;
        const float invz = 1.0f / C2.at<float>(2);
        const float ex_ = KF[1].fx * C2.at<float>(0) * invz + KF[1].cx, ey_ = KF[1].fy * C2.at<float>(1) * invz + KF[1].cy;
        std::vector<uint8_t> h1(nA + 1, 0), h2(nB + 1, 0);
        for (int i = 0; i < nA; i++) h1[i] = KF[0].mvpMapPoints[i] != nullptr;
        for (int i = 0; i < nB; i++) h2[i] = KF[1].mvpMapPoints[i] != nullptr;
        std::vector<int> pairs(2 * (nA + 1));
        const int onp = oracle_search_for_triangulation(0, 0, nA, fe[0].desc.data, okA, h1.data(), KF[0].mvuRight.data(),
                                                        fvA.fv, nB, fe[1].desc.data, okB, h2.data(), KF[1].mvuRight.data(),
                                                        fvB.fv, Fv, ex_, ey_, scale.data(), sigma2.data(), pairs.data(),
                                                        nA + 1);
        bool ok = nm == onp && (int)v.size() == onp;
        for (int i = 0; ok && i < onp; i++)
            ok = v[i].first == (size_t)pairs[2 * i] && v[i].second == (size_t)pairs[2 * i + 1];
        const double g = median_us([&] { m.SearchForTriangulation(&KF[0], &KF[1], F12, v, false); }, reps);
        const double c = median_us([&] {
            oracle_search_for_triangulation(0, 0, nA, fe[0].desc.data, okA, h1.data(), KF[0].mvuRight.data(), fvA.fv, nB,
                                            fe[1].desc.data, okB, h2.data(), KF[1].mvuRight.data(), fvB.fv, Fv, ex_, ey_,
                                            scale.data(), sigma2.data(), pairs.data(), nA + 1);
        }, cpu_reps);
        emit("SearchForTriangulation", g, c, nm, onp, ok);
        // LocalMapping's neighbour loop (LocalMapping.cc:247-278) as one batched call: KF1 against kNeigh KF2s (the
        // second keyframe each time: the same work per pair), against kNeigh runs of the CPU loop
        constexpr int kNeigh = 10;
        std::vector<KeyFrame*> vpKF2(kNeigh, &KF[1]);
        std::vector<cv::Mat> vF12(kNeigh, F12);
        std::vector<std::vector<std::pair<size_t, size_t> > > vv;
        const int tot = m.SearchForTriangulation(&KF[0], vpKF2, vF12, vv, false);
        bool bok = (int)vv.size() == kNeigh && tot == kNeigh * onp;
        for (int p = 0; bok && p < kNeigh; p++) bok = vv[p] == v;
        const double gb = median_us([&] { m.SearchForTriangulation(&KF[0], vpKF2, vF12, vv, false); }, reps);
        emit("SearchForTriangulation_x10", gb, kNeigh * c, tot, kNeigh * onp, bok && ok);
    }
    // ---- SearchForInitialization (window 100; vbPrevMatched = the first frame's keypoints)
    {
        ORBmatcher m(0.9f, true);
        std::vector<cv::Point2f> prev0(nA);
        for (int i = 0; i < nA; i++) prev0[i] = fe[0].kps[i].pt;
        std::vector<cv::Point2f> prev = prev0;
        std::vector<int> v;
        const int nm = m.SearchForInitialization(F[0], F[1], prev, v, 100);
        // the CPU loop: the reference's per-keypoint grid query (level 0 only, :421-426) + the restated body
        std::vector<int> off(nA + 1, 0), cand, om(nA + 1, -1);
        auto cpu = [&]() {
            cand.clear();
            for (int i = 0; i < nA; i++) {
                if (fe[0].kps[i].octave == 0) {
                    const std::vector<size_t> c = F[1].GetFeaturesInArea(prev0[i].x, prev0[i].y, 100.f, 0, 0);
                    for (size_t j : c) cand.push_back((int)j);
                }
                off[i + 1] = (int)cand.size();
            }
            if (cand.empty()) cand.push_back(0);
            return oracle_window_match(0.9f, 1, 1, nA, fe[0].desc.data, okA, nB, fe[1].desc.data, okB, off.data(),
                                       cand.data(), om.data());
        };
        const int onm = cpu();
        bool ok = nm == onm && (int)v.size() == nA;
        for (int i = 0; ok && i < nA; i++) ok = v[i] == om[i];
        const double g = median_us([&] {
            std::vector<cv::Point2f> p = prev0;
            m.SearchForInitialization(F[0], F[1], p, v, 100);
        }, reps);
        const double c = median_us([&] { cpu(); }, cpu_reps);
        emit("SearchForInitialization", g, c, nm, onm, ok);
    }
    // ---- Frame::ComputeBoW: vocabulary transform of one frame's descriptors, levelsup 4
    {
        void* ov = oracle_vocab_load(argv[5]);
        int k = 0, L = 0, sc = 0, wt = 0, nn = 0, nw = 0;
        oracle_vocab_info(ov, &k, &L, &sc, &wt, &nn, &nw);
        std::vector<int> bw(nB + 1), fo(nB + 2), fi(nB + 1);
        std::vector<uint32_t> fn(nB + 1);
        std::vector<double> bv(nB + 1);
        int nb = 0, nf = 0;
        BowVector gbv;
        BowFeatureVector gfv;
        voc.transform(descs[1], gbv, gfv, 4);
        oracle_vocab_transform(ov, fe[1].desc.data, nB, 4, bw.data(), bv.data(), &nb, fn.data(), fo.data(),
                               fi.data(), &nf);
        bool ok = (int)gbv.size() == nb && (int)gfv.size() == nf;
        int j = 0;
        for (auto it = gfv.begin(); ok && it != gfv.end(); ++it, ++j)
            ok = it->first == fn[j] && (int)it->second.size() == fo[j + 1] - fo[j];
        const double g = median_us([&] { voc.transform(descs[1], gbv, gfv, 4); }, reps);
        const double c = median_us([&] {
            oracle_vocab_transform(ov, fe[1].desc.data, nB, 4, bw.data(), bv.data(), &nb, fn.data(),
                                   fo.data(), fi.data(), &nf);
        }, cpu_reps);
        oracle_vocab_destroy(ov);
        emit("ComputeBoW", g, c, (int)gfv.size(), nf, ok);
        snprintf(buf, sizeof buf, ", \"vocabulary\": {\"k\": %d, \"L\": %d, \"nodes\": %d, \"words\": %d, \"levelsup\": 4, "
                 "\"featvec_nodes\": [%d, %d]}", k, L, nn, nw, (int)fe[0].fv.size(), (int)fe[1].fv.size());
        out += buf;
    }
    // ---- Frame::ComputeStereoMatches on a rectified pair (frames 2 and 3): the two extractors ran on the left
    // and right images (the stereo Frame ctor, Frame.cc:124-127), then the search (:141 -> :662-836)
    if (with_stereo) {
        ORBextractor exL(nfeat, 1.2f, 8, 20, 7, 0), exR(nfeat, 1.2f, 8, 20, 7, 0);
        std::vector<ORB_SLAM2::KeyPoint> kL, kR;
        DescriptorMat dL, dR;
        const uint8_t* imL = frames.data() + (size_t)2 * w * h;
        const uint8_t* imR = frames.data() + (size_t)3 * w * h;
        exL(ImageView(imL, w, h), ImageView(), kL, dL);
        exR(ImageView(imR, w, h), ImageView(), kR, dR);
        const float mb = 0.54f, mbf = 0.54f * 721.5f;   // KITTI-like baseline / baseline x fx
        std::vector<float> ur, dp;
        const int nm = ComputeStereoMatches(exL, exR, kL, dL, kR, dR, mb, mbf, ur, dp);
        void* oL = oracle_create(nfeat, 1.2f, 8, 20, 7, 0);
        void* oR = oracle_create(nfeat, 1.2f, 8, 20, 7, 0);
        oracle_run(oL, imL, w, h, w);
        oracle_run(oR, imR, w, h, w);
        const int nL = (int)kL.size(), nR = (int)kR.size();
        std::vector<float> our(nL + 1), odp(nL + 1);
        const OracleKeyPoint* okL = reinterpret_cast<const OracleKeyPoint*>(kL.data());
        const OracleKeyPoint* okR = reinterpret_cast<const OracleKeyPoint*>(kR.data());
        const int onm = oracle_stereo_matches(oL, oR, nL, okL, dL.buf.data(), nR, okR, dR.buf.data(), mb, mbf,
                                              our.data(), odp.data());
        bool ok = nm == onm && (int)ur.size() == nL && (int)dp.size() == nL;
        for (int i = 0; ok && i < nL; i++) ok = memcmp(&ur[i], &our[i], 4) == 0 && memcmp(&dp[i], &odp[i], 4) == 0;
        const double g = median_us([&] { ComputeStereoMatches(exL, exR, kL, dL, kR, dR, mb, mbf, ur, dp); }, reps);
        const double c = median_us([&] {
            oracle_stereo_matches(oL, oR, nL, okL, dL.buf.data(), nR, okR, dR.buf.data(), mb, mbf, our.data(), odp.data());
        }, cpu_reps);
        oracle_destroy(oL);
        oracle_destroy(oR);
        emit("ComputeStereoMatches", g, c, nm, onm, ok);
    }
    // ---- SearchByMatchBird, both forms: frame 0's features as the keyframe's / last frame's birdview keypoints (70 %
    // of them with a MapPointBird, whose descriptor is the keypoint's), frame 1's as the current frame's
    if (argc > 8 && !strcmp(argv[8], "bird")) {
        orb_params prm;   // a matcher context, as the host mirror creates it
        memset(&prm, 0, sizeof prm);
        prm.nfeatures = 1000;
        prm.scaleFactor = 1.2f;
        prm.nlevels = 8;
        prm.iniThFAST = 20;
        prm.minThFAST = 7;
        prm.device = getenv("ORBGPU_DEVICE") ? atoi(getenv("ORBGPU_DEVICE")) : 0;
        int err = 0;
        orb_ctx* ctx = orb_create(&prm, &err);
        if (!ctx) {
            fprintf(stderr, "bird leg: no context (%d)\n", err);
            return 2;
        }
        const Frame& Fc = F[1];
        std::vector<int> off(FRAME_GRID_COLS * FRAME_GRID_ROWS + 1, 0), idx;
        for (int ix = 0; ix < FRAME_GRID_COLS; ix++)
            for (int iy = 0; iy < FRAME_GRID_ROWS; iy++) {
                for (size_t j : Fc.mGrid[ix][iy]) idx.push_back((int)j);
                off[ix * FRAME_GRID_ROWS + iy + 1] = (int)idx.size();
            }
        if (idx.empty()) idx.push_back(0);
        const orb_frame_grid g = {0.f, 0.f, Fc.mfGridElementWidthInv, Fc.mfGridElementHeightInv, off.data(), idx.data()};
        std::vector<uint8_t> has(nA + 1, 0);
        std::vector<int> qid;
        std::vector<float> qxy, qang;
        std::vector<uint8_t> qd;
        uint32_t s = 77u;
        for (int k = 0; k < nA; k++) {
            if (lcg(s) % 10 >= 7) continue;
            has[k] = 1;
            qid.push_back(k);
            qxy.push_back(fe[0].kps[k].pt.x);
            qxy.push_back(fe[0].kps[k].pt.y);
            qang.push_back(fe[0].kps[k].angle);
            qd.insert(qd.end(), fe[0].desc.data + (size_t)k * 32, fe[0].desc.data + (size_t)k * 32 + 32);
        }
        const int nq = (int)qid.size();
        const float nnr = 0.99f, r = 15.f;
        const orb_keypoint* kA = reinterpret_cast<const orb_keypoint*>(fe[0].kps.data());
        const orb_keypoint* kB = reinterpret_cast<const orb_keypoint*>(fe[1].kps.data());
        std::vector<int> gm(nB + 1, -1), cm(nB + 1, -1);
        int gn = 0;
        auto gpu_kf = [&] {
            return orb_search_by_match_bird(ctx, nnr, 1, 100, r, nq, qid.data(), qxy.data(), qang.data(), qd.data(), nB,
                                            fe[1].desc.data, kB, g, gm.data(), &gn);
        };
        auto cpu_kf = [&] {   // ORBmatcher.cc:2000-2114
            std::fill(cm.begin(), cm.end(), -1);
            std::vector<int> vMatchedDistanceBird(nB, INT_MAX), hist[30];
            int nmatches = 0;
            for (int i = 0; i < nq; i++) {
                const float x = qxy[2 * i], y = qxy[2 * i + 1];
                const std::vector<size_t> vIndices = Fc.GetFeaturesInArea(x, y, r);
                if (vIndices.empty()) continue;
                int bestDist = INT_MAX, bestLevel = -1, bestDist2 = INT_MAX, bestLevel2 = -1, bestIdx = -1;
                for (size_t id : vIndices) {
                    const int dist = oracle_descriptor_distance(&qd[(size_t)i * 32], fe[1].desc.data + id * 32);
                    if (vMatchedDistanceBird[id] <= dist) continue;
                    if (dist < bestDist) {
                        bestDist2 = bestDist;
                        bestDist = dist;
                        bestLevel2 = bestLevel;
                        bestLevel = fe[1].kps[id].octave;
                        bestIdx = (int)id;
                    } else if (dist < bestDist2) {
                        bestLevel2 = fe[1].kps[id].octave;
                        bestDist2 = dist;
                    }
                }
                if (bestDist <= 100 && (bestLevel != bestLevel2 || bestDist < (float)bestDist2 * nnr)) {
                    cm[bestIdx] = qid[i];
                    vMatchedDistanceBird[bestIdx] = bestDist;
                    hist[oracle_rot_bin(qang[i], fe[1].kps[bestIdx].angle)].push_back(bestIdx);
                    nmatches++;
                }
            }
            int sizes[30], i1 = -1, i2 = -1, i3 = -1;
            for (int b = 0; b < 30; b++) sizes[b] = (int)hist[b].size();
            oracle_three_maxima(sizes, 30, &i1, &i2, &i3);
            for (int b = 0; b < 30; b++) {
                if (b == i1 || b == i2 || b == i3) continue;
                for (int t : hist[b]) {
                    cm[t] = -2;
                    nmatches--;
                }
            }
            return nmatches;
        };
        if (gpu_kf() != ORB_OK) return fprintf(stderr, "orb_search_by_match_bird: %s\n", orb_last_error()), 2;
        int cn = cpu_kf();
        bool ok = gn == cn && std::equal(gm.begin(), gm.begin() + nB, cm.begin());
        double gt = median_us([&] { gpu_kf(); }, reps), ct = median_us([&] { cpu_kf(); }, cpu_reps);
        emit("SearchByMatchBird_KF_F", gt, ct, gn, cn, ok);
        // the frame form: BirdviewMatch(LastFrame, CurrentFrame, 15) + the carry-over
        auto gpu_f = [&] {
            return orb_search_by_match_bird_frame(ctx, nnr, 1, 15.f, nA, fe[0].desc.data, kA, has.data(), nB,
                                                  fe[1].desc.data, kB, g, gm.data(), &gn);
        };
        std::vector<int> coff(nA + 1, 0), cand, m12(nA + 1, -1);
        auto cpu_f = [&] {   // :1790-1921: the per-keypoint grid query on the query's own octave + the restated body
            cand.clear();
            for (int i = 0; i < nA; i++) {
                const int lv = fe[0].kps[i].octave;
                for (size_t j : Fc.GetFeaturesInArea(fe[0].kps[i].pt.x, fe[0].kps[i].pt.y, 15.f, lv, lv)) cand.push_back((int)j);
                coff[i + 1] = (int)cand.size();
            }
            if (cand.empty()) cand.push_back(0);
            oracle_window_match(nnr, 1, 0, nA, fe[0].desc.data, okA, nB, fe[1].desc.data, okB, coff.data(), cand.data(),
                                m12.data());
            std::fill(cm.begin(), cm.end(), -1);
            int nmatches = 0;
            for (int k = 0; k < nA; k++)
                if (m12[k] >= 0 && has[k]) {
                    cm[m12[k]] = k;
                    nmatches++;
                }
            return nmatches;
        };
        if (gpu_f() != ORB_OK) return fprintf(stderr, "orb_search_by_match_bird_frame: %s\n", orb_last_error()), 2;
        cn = cpu_f();
        ok = gn == cn && std::equal(gm.begin(), gm.begin() + nB, cm.begin());
        gt = median_us([&] { gpu_f(); }, reps);
        ct = median_us([&] { cpu_f(); }, cpu_reps);
        emit("SearchByMatchBird_F_F", gt, ct, gn, cn, ok);
        snprintf(buf, sizeof buf, ", \"bird_queries\": %d", nq);
        out += buf;
        orb_destroy(ctx);
    }
    snprintf(buf, sizeof buf, ", \"keypoints\": [%d, %d], \"gpu_reps\": %d, \"cpu_reps\": %d, \"all_equal\": %s}", nA, nB,
             reps, cpu_reps, all_ok ? "true" : "false");
    out += buf;
    printf("%s\n", out.c_str());
    for (MapPoint* p : pool) delete p;
    return all_ok ? 0 : 1;
}
