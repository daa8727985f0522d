// Runs the host mirror's colour operator(), ComputeStereoFromRGBD and ResidentFrame::FromBatchRGBD:
//   test_rgbd_mirror <case.bin> <results.bin>
// case.bin (little endian, written by tests/test_gpu_rgbd.py):
//   float fx, fy, cx, cy, k[4] | int32 w, h, nframes, kp_cap | float mbf, factor | nframes int32 counts |
//   nframes * kp_cap keypoints (raw) | nframes * kp_cap descriptors (orb_extract_batch_device's output layout) |
//   nframes w x h uint16 depth images | one w x h BGR image
// results.bin: colour extraction of the BGR image: int32 n, n keypoints, n descriptors, w * h bytes mvImagePyramid[0] |
//   ComputeStereoFromRGBD of frame 0 (keypoints undistorted by UndistortKeyPoints): int32 N, int32 nvalid, N floats
//   mvuRight, N floats mvDepth | FromBatchRGBD: per frame int32 hasURight, int32 N, 3,073 int32 cell_off, int32 nslots,
//   nslots int32 cell_idx | nframes * kp_cap floats d_uRight | nframes * kp_cap floats d_depth
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../orb-slam-birdview_amd/host/ORBmatcher.h"
#include "../../orb-slam-birdview_amd/host/Stereo.h"

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
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return fprintf(stderr, "usage: %s case.bin results.bin\n", argv[0]), 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    void *d_kps = nullptr, *d_desc = nullptr, *d_counts = nullptr, *d_map = nullptr, *d_ur = nullptr, *d_dep = nullptr;
    orb_ctx* ctx = nullptr;
    int rc = 0;
    try {
        const std::vector<float> cal = rd<float>(8);
        const std::vector<int32_t> head = rd<int32_t>(4);
        const int w = head[0], h = head[1], nframes = head[2], kp_cap = head[3];
        const std::vector<float> par = rd<float>(2);
        const float mbf = par[0], factor = par[1];
        if (nframes < 1 || kp_cap < 1) return fprintf(stderr, "the case holds at least one frame\n"), 2;
        const std::vector<int32_t> counts = rd<int32_t>(nframes);
        const std::vector<KeyPoint> keys = rd<KeyPoint>((size_t)nframes * kp_cap);
        const std::vector<uint8_t> desc = rd<uint8_t>((size_t)nframes * kp_cap * 32);
        const std::vector<uint16_t> depth = rd<uint16_t>((size_t)nframes * w * h);
        const std::vector<uint8_t> bgr = rd<uint8_t>((size_t)w * h * 3);

        ORBextractor ext(500, 1.2f, 8, 20, 7);
        ctx = ext.context();
        {   // the camera's colour image through the extractor
            std::vector<KeyPoint> k;
            DescriptorMat d;
            ext(ColorImageView(bgr.data(), w, h, 0, ORB_COLOR_BGR), ImageView(), k, d);
            const int32_t n = (int32_t)k.size();
            fwrite(&n, 4, 1, out);
            if (n) fwrite(k.data(), sizeof(KeyPoint), k.size(), out);
            if (n) fwrite(d.buf.data(), 32, k.size(), out);
            const ImageView& g = ext.mvImagePyramid[0];
            if (g.cols != w || g.rows != h) return fprintf(stderr, "mvImagePyramid[0] is %d x %d\n", g.cols, g.rows), 1;
            for (int y = 0; y < h; y++) fwrite(g.data + (size_t)y * g.step, 1, w, out);
        }
        float b[4];
        ComputeImageBounds(cal[0], cal[1], cal[2], cal[3], &cal[4], w, h, b[0], b[1], b[2], b[3]);
        orb_depth_map map;
        map.data = depth.data();
        map.type = ORB_DEPTH_U16;
        map.w = w;
        map.h = h;
        map.row_stride = (size_t)w * 2;
        map.frame_pitch = (size_t)w * h * 2;
        map.factor = factor;
        {   // one frame whose keypoints are on the host
            const std::vector<KeyPoint> keys0(keys.begin(), keys.begin() + counts[0]);
            const std::vector<KeyPoint> un0 = UndistortKeyPoints(cal[0], cal[1], cal[2], cal[3], &cal[4], keys0);
            std::vector<float> ur, dep;
            const int32_t nv = ComputeStereoFromRGBD(map, keys0, un0, mbf, ur, dep), n0 = (int32_t)keys0.size();
            fwrite(&n0, 4, 1, out);
            fwrite(&nv, 4, 1, out);
            if (n0) fwrite(ur.data(), 4, ur.size(), out);
            if (n0) fwrite(dep.data(), 4, dep.size(), out);
        }
        // the batch on the device, as an extraction leaves it
        const size_t total = (size_t)nframes * kp_cap;
        d_kps = orb_device_alloc(ctx, keys.size() * sizeof(KeyPoint));
        d_desc = orb_device_alloc(ctx, desc.size());
        d_counts = orb_device_alloc(ctx, counts.size() * 4);
        d_map = orb_device_alloc(ctx, depth.size() * 2);
        d_ur = orb_device_alloc(ctx, total * 4);
        d_dep = orb_device_alloc(ctx, total * 4);
        if (!d_kps || !d_desc || !d_counts || !d_map || !d_ur || !d_dep ||
            orb_memcpy_h2d(ctx, d_kps, keys.data(), keys.size() * sizeof(KeyPoint)) ||
            orb_memcpy_h2d(ctx, d_desc, desc.data(), desc.size()) ||
            orb_memcpy_h2d(ctx, d_counts, counts.data(), counts.size() * 4) ||
            orb_memcpy_h2d(ctx, d_map, depth.data(), depth.size() * 2) || orb_memset_device(ctx, d_ur, 0, total * 4) ||
            orb_memset_device(ctx, d_dep, 0, total * 4))
            return fprintf(stderr, "upload failed\n"), 1;
        orb_distortion dist;
        dist.fx = cal[0];
        dist.fy = cal[1];
        dist.cx = cal[2];
        dist.cy = cal[3];
        for (int k = 0; k < 4; k++) dist.k[k] = cal[4 + k];
        map.data = d_map;
        {
            std::vector<ResidentFrame> all = ResidentFrame::FromBatchRGBD(
                ctx, dist, map, mbf, nframes, (const uint8_t*)d_desc, (const KeyPoint*)d_kps, (const int*)d_counts, kp_cap,
                b[0], b[1], b[2], b[3], (float*)d_ur, (float*)d_dep);
            if ((int)all.size() != nframes) return fprintf(stderr, "FromBatchRGBD: %zu frames\n", all.size()), 1;
            for (const ResidentFrame& R : all) {
                std::vector<int> off, idx;
                R.Grid(off, idx);
                const int32_t has = R.hasURight() ? 1 : 0, n = R.N(), ns = (int32_t)idx.size();
                fwrite(&has, 4, 1, out);
                fwrite(&n, 4, 1, out);
                fwrite(off.data(), 4, off.size(), out);
                fwrite(&ns, 4, 1, out);
                if (ns) fwrite(idx.data(), 4, idx.size(), out);
            }
            std::vector<float> ur(total), dep(total);
            if (orb_memcpy_d2h(ctx, ur.data(), d_ur, total * 4) || orb_memcpy_d2h(ctx, dep.data(), d_dep, total * 4))
                return fprintf(stderr, "download failed\n"), 1;
            fwrite(ur.data(), 4, total, out);
            fwrite(dep.data(), 4, total, out);
            // a failing batch throws and leaves nothing behind
            bool threw = false;
            try {
                map.type = 9;
                ResidentFrame::FromBatchRGBD(ctx, dist, map, mbf, nframes, (const uint8_t*)d_desc, (const KeyPoint*)d_kps,
                                             (const int*)d_counts, kp_cap, b[0], b[1], b[2], b[3], nullptr, nullptr);
            } catch (const OrbGpuError&) {
                threw = true;
            }
            if (!threw) return fprintf(stderr, "an unknown depth type was accepted\n"), 1;
        }   // (the frames die before their context)
        for (void* p : {d_kps, d_desc, d_counts, d_map, d_ur, d_dep}) orb_device_free(ctx, p);
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        rc = 1;
    }
    fclose(out);
    return rc;
}
