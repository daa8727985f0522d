// Runs the host mirror's Rectifier (remap of both eyes; operator() on a raw pair) and ComputeStereoMatches behind it:
//   test_rectify_mirror <case.bin> <results.bin> <nlevels>
// case.bin (little endian, written by tests/test_gpu_stereo_frames.py):
//   int32 w, h | float mb, mbf | four w x h float maps (M1l, M2l, M1r, M2r) | the raw left and right images, w x h bytes
// results.bin: imLeftRect, imRightRect (w * h bytes each) | left: int32 n, n keypoints, n descriptors | right likewise |
//   int32 nmatched, N floats mvuRight, N floats mvDepth (N = left n)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../orb-slam-birdview_amd/host/Rectifier.h"
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
    if (argc != 4 || !(in = fopen(argv[1], "rb")))
        return fprintf(stderr, "usage: %s case.bin results.bin nlevels\n", argv[0]), 2;
    const int nlevels = atoi(argv[3]);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    int rc = 0;
    try {
        const std::vector<int32_t> head = rd<int32_t>(2);
        const int w = head[0], h = head[1];
        const std::vector<float> par = rd<float>(2);
        const size_t px = (size_t)w * h;
        const std::vector<float> m1l = rd<float>(px), m2l = rd<float>(px), m1r = rd<float>(px), m2r = rd<float>(px);
        const std::vector<uint8_t> rawL = rd<uint8_t>(px), rawR = rd<uint8_t>(px);

        ORBextractor left(500, 1.2f, nlevels, 20, 7), right(500, 1.2f, nlevels, 20, 7);
        {
            Rectifier rect(left.context(), MapView(m1l.data(), m2l.data(), w, h), MapView(m1r.data(), m2r.data(), w, h));
            if (rect.cols() != w || rect.rows() != h) return fprintf(stderr, "Rectifier is %d x %d\n", rect.cols(), rect.rows()), 1;
            std::vector<uint8_t> imRect;
            rect.remap(Rectifier::LEFT, ImageView(rawL.data(), w, h), imRect);
            fwrite(imRect.data(), 1, imRect.size(), out);
            rect.remap(Rectifier::RIGHT, ImageView(rawR.data(), w, h), imRect);
            fwrite(imRect.data(), 1, imRect.size(), out);

            std::vector<KeyPoint> kl, kr;
            DescriptorMat dl, dr;
            rect(left, right, ImageView(rawL.data(), w, h), ImageView(rawR.data(), w, h), kl, dl, kr, dr);
            const std::vector<KeyPoint>* ks[2] = {&kl, &kr};
            const DescriptorMat* ds[2] = {&dl, &dr};
            for (int e = 0; e < 2; e++) {
                const int32_t n = (int32_t)ks[e]->size();
                fwrite(&n, 4, 1, out);
                if (n) fwrite(ks[e]->data(), sizeof(KeyPoint), n, out);
                if (n) fwrite(ds[e]->buf.data(), 32, n, out);
            }
            std::vector<float> ur, depth;
            const int32_t nm = ComputeStereoMatches(left, right, kl, dl, kr, dr, par[0], par[1], ur, depth);
            fwrite(&nm, 4, 1, out);
            if (!ur.empty()) fwrite(ur.data(), 4, ur.size(), out);
            if (!depth.empty()) fwrite(depth.data(), 4, depth.size(), out);
        }   // (the Rectifier goes before the extractor whose context created it)
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    fclose(out);
    return rc;
}
