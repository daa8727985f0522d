// Runs the host mirror's UndistortKeyPoints, ComputeImageBounds and the ResidentFrame factories over an extraction's
// output slots:
//   test_undistort_mirror <case.bin> <results.bin>
// case.bin (little endian, written by tests/test_gpu_undistort_mirror.py):
//   float fx, fy, cx, cy, k[4] | int32 w, h, nframes, kp_cap | nframes int32 counts | nframes * kp_cap keypoints (raw) |
//   nframes * kp_cap descriptors: the layout of orb_extract_batch_device's outputs, uploaded here as they are
// results.bin: float bounds[4] | int32 counts[0] | counts[0] keypoints: UndistortKeyPoints of frame 0's |
//   FromExtraction(frame 1's slot): int32 N, 3,073 int32 cell_off, int32 nslots, nslots int32 cell_idx |
//   FromBatch: the same four per frame.
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
void wr_frame(FILE* out, const ResidentFrame& R) {
    std::vector<int> off, idx;
    R.Grid(off, idx);
    const int32_t n = R.N(), ns = (int32_t)idx.size();
    fwrite(&n, 4, 1, out);
    fwrite(off.data(), 4, off.size(), out);
    fwrite(&ns, 4, 1, out);
    if (ns) fwrite(idx.data(), 4, idx.size(), out);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return fprintf(stderr, "usage: %s case.bin results.bin\n", argv[0]), 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    orb_ctx* ctx = nullptr;
    void *d_kps = nullptr, *d_desc = nullptr, *d_counts = nullptr;
    int rc = 0;
    try {
        const std::vector<float> cal = rd<float>(8);
        const std::vector<int32_t> head = rd<int32_t>(4);
        const int w = head[0], h = head[1], nframes = head[2], kp_cap = head[3];
        if (nframes < 2 || kp_cap < 1) return fprintf(stderr, "the case holds at least two frames\n"), 2;
        const std::vector<int32_t> counts = rd<int32_t>(nframes);
        const std::vector<KeyPoint> keys = rd<KeyPoint>((size_t)nframes * kp_cap);
        const std::vector<uint8_t> desc = rd<uint8_t>((size_t)nframes * kp_cap * 32);
        float b[4];
        ComputeImageBounds(cal[0], cal[1], cal[2], cal[3], &cal[4], w, h, b[0], b[1], b[2], b[3]);
        fwrite(b, 4, 4, out);
        const std::vector<KeyPoint> keys0(keys.begin(), keys.begin() + counts[0]);
        const std::vector<KeyPoint> un0 = UndistortKeyPoints(cal[0], cal[1], cal[2], cal[3], &cal[4], keys0);
        const int32_t n0 = (int32_t)un0.size();
        fwrite(&n0, 4, 1, out);
        if (n0) fwrite(un0.data(), sizeof(KeyPoint), un0.size(), out);

        // the slots on the device, as an extraction leaves them
        orb_params p = {};
        p.nfeatures = 500;
        p.scaleFactor = 1.2f;
        p.nlevels = 8;
        p.iniThFAST = 20;
        p.minThFAST = 7;
        int st = 0;
        ctx = orb_create(&p, &st);
        if (!ctx) return fprintf(stderr, "orb_create: %d\n", st), 1;
        d_kps = orb_device_alloc(ctx, keys.size() * sizeof(KeyPoint));
        d_desc = orb_device_alloc(ctx, desc.size());
        d_counts = orb_device_alloc(ctx, counts.size() * 4);
        if (!d_kps || !d_desc || !d_counts || orb_memcpy_h2d(ctx, d_kps, keys.data(), keys.size() * sizeof(KeyPoint)) ||
            orb_memcpy_h2d(ctx, d_desc, desc.data(), desc.size()) ||
            orb_memcpy_h2d(ctx, d_counts, counts.data(), counts.size() * 4))
            return fprintf(stderr, "upload failed\n"), 1;
        orb_distortion dist;
        dist.fx = cal[0];
        dist.fy = cal[1];
        dist.cx = cal[2];
        dist.cy = cal[3];
        for (int k = 0; k < 4; k++) dist.k[k] = cal[4 + k];
        {
            ResidentFrame one = ResidentFrame::FromExtraction(
                ctx, dist, counts[1], (const uint8_t*)d_desc + (size_t)kp_cap * 32, (const KeyPoint*)d_kps + kp_cap,
                nullptr, b[0], b[1], b[2], b[3]);
            wr_frame(out, one);
            std::vector<ResidentFrame> all = ResidentFrame::FromBatch(ctx, dist, nframes, (const uint8_t*)d_desc,
                                                                      (const KeyPoint*)d_kps, (const int*)d_counts,
                                                                      kp_cap, b[0], b[1], b[2], b[3]);
            if ((int)all.size() != nframes) return fprintf(stderr, "FromBatch: %zu frames\n", all.size()), 1;
            for (const ResidentFrame& R : all) wr_frame(out, R);
            // a failing batch throws and leaves nothing behind
            bool threw = false;
            try {
                ResidentFrame::FromBatch(ctx, dist, nframes, (const uint8_t*)d_desc, (const KeyPoint*)d_kps,
                                         (const int*)d_counts, 0, b[0], b[1], b[2], b[3]);
            } catch (const OrbGpuError&) {
                threw = true;
            }
            if (!threw) return fprintf(stderr, "kp_cap = 0 was accepted\n"), 1;
        }   // (the frames die before their context)
    } catch (const OrbGpuError& e) {
        fprintf(stderr, "OrbGpuError: %s\n", e.what());
        rc = 1;
    }
    if (ctx) {
        orb_device_free(ctx, d_kps);
        orb_device_free(ctx, d_desc);
        orb_device_free(ctx, d_counts);
        orb_destroy(ctx);
    }
    fclose(out);
    return rc;
}
