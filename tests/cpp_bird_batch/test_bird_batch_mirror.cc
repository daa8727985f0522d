// Drives the host mirror's BirdviewORB::extractBirdviewBatch the way a caller with queued frames would:
//   test_bird_batch_mirror <frames.bin> <results.bin>
// frames.bin (little endian, written by tests/test_gpu_bird_batch_mirror.py):
//   int32 nfeatures | int32 w | int32 h | int32 nframes | int32 nmasks | nframes images (w*h B) | nmasks masks (w*h B)
// The program calls extractBirdviewBatch three times on one object: with no mask, with masks[0] shared, and
// with all nmasks (== nframes) masks.
// results.bin: per call, per frame: int32 n | n keypoints (28 B) | n descriptors (32 B).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../orb-slam-birdview_amd/host/BirdviewORB.h"

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
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return fprintf(stderr, "usage: %s frames.bin results.bin\n", argv[0]), 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    try {
        const std::vector<int32_t> hd = rd<int32_t>(5);
        const int nfeatures = hd[0], w = hd[1], h = hd[2], nf = hd[3], nm = hd[4];
        if (nm != nf) return fprintf(stderr, "one mask per frame expected\n"), 2;
        const std::vector<uint8_t> imgs = rd<uint8_t>((size_t)nf * w * h), masks = rd<uint8_t>((size_t)nm * w * h);
        const std::vector<uint8_t> masks0 = masks;
        std::vector<ImageView> iv, mv;
        for (int f = 0; f < nf; f++) iv.emplace_back(imgs.data() + (size_t)f * w * h, w, h);
        for (int m = 0; m < nm; m++) mv.emplace_back(masks.data() + (size_t)m * w * h, w, h);
        auto orb = BirdviewORB::create(nfeatures);
        for (int call = 0; call < 3; call++) {
            std::vector<ImageView> use;
            if (call == 1) use.assign(mv.begin(), mv.begin() + 1);
            if (call == 2) use = mv;
            std::vector<std::vector<KeyPoint>> keys;
            std::vector<DescriptorMat> desc;
            orb->extractBirdviewBatch(iv, use, keys, desc);
            if ((int)keys.size() != nf || (int)desc.size() != nf) return fprintf(stderr, "result count\n"), 1;
            for (int f = 0; f < nf; f++) {
                const int32_t n = (int32_t)keys[f].size();
                if (desc[f].rows != n) return fprintf(stderr, "descriptor rows\n"), 1;
                fwrite(&n, 4, 1, out);
                fwrite(keys[f].data(), sizeof(KeyPoint), n, out);
                fwrite(desc[f].buf.data(), 32, n, out);
            }
        }
        if (masks != masks0) return fprintf(stderr, "the masks were modified\n"), 1;
        // 2 masks for nf >= 3 frames is an argument error, thrown before any work
        if (nf >= 3) {
            std::vector<ImageView> two(mv.begin(), mv.begin() + 2);
            std::vector<std::vector<KeyPoint>> keys;
            std::vector<DescriptorMat> desc;
            bool thrown = false;
            try {
                orb->extractBirdviewBatch(iv, two, keys, desc);
            } catch (const OrbGpuError&) {
                thrown = true;
            }
            if (!thrown) return fprintf(stderr, "2 masks for %d frames did not throw\n", nf), 1;
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    fclose(out);
    return 0;
}
