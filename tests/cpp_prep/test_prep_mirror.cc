// Runs the host mirror's FrontPrep (operator() on a raw gray and a raw colour frame) and ConvertMaskBirdview:
//   test_prep_mirror <case.bin> <results.bin>
// case.bin (little endian, written by tests/test_gpu_prep.py):
//   int32 sw, sh, cx, cy, cw, ch, mask_channels, code, nlevels, bw, bh |
//   the camera mask, sw x sh x mask_channels | a gray frame, sw x sh | a colour frame of `code`, sw x sh x 3 or 4 |
//   a birdview mask image, bw x bh x 3
// results.bin: int32 cols, rows | for the gray, then the colour frame: int32 n, n keypoints, n descriptors,
//   mvImagePyramid[0] (cols * rows bytes, rows packed) | ConvertMaskBirdview's output, bw * bh bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <stdexcept>
#include <vector>

#include "../../orb-slam-birdview_amd/host/FrontPrep.h"

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

void put(FILE* out, ORBextractor& e, const std::vector<KeyPoint>& k, const DescriptorMat& d, int cols, int rows) {
    const int32_t n = (int32_t)k.size();
    fwrite(&n, 4, 1, out);
    if (n) fwrite(k.data(), sizeof(KeyPoint), n, out);
    if (n) fwrite(d.buf.data(), 32, n, out);
    const ImageView& l0 = e.mvImagePyramid[0];
    if (l0.cols != cols || l0.rows != rows) {
        fprintf(stderr, "mvImagePyramid[0] is %d x %d\n", l0.cols, l0.rows);
        exit(1);
    }
    for (int y = 0; y < rows; y++) fwrite(l0.data + (size_t)y * l0.step, 1, cols, out);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return fprintf(stderr, "usage: %s case.bin results.bin\n", argv[0]), 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    int rc = 0;
    try {
        const std::vector<int32_t> hd = rd<int32_t>(11);
        const int sw = hd[0], sh = hd[1], mc = hd[6], code = hd[7], nlevels = hd[8], bw = hd[9], bh = hd[10];
        const int C = (code == ORB_COLOR_RGB || code == ORB_COLOR_BGR) ? 3 : 4;
        const size_t px = (size_t)sw * sh;
        const std::vector<uint8_t> mask = rd<uint8_t>(px * mc), gray = rd<uint8_t>(px), colour = rd<uint8_t>(px * C);
        const std::vector<uint8_t> bird = rd<uint8_t>((size_t)bw * bh * 3);

        ORBextractor ext(500, 1.2f, nlevels, 20, 7);
        {
            FrontPrep prep(ext.context(), sw, sh, MaskView(mask.data(), sw, sh, 0, mc), CropRect(hd[2], hd[3], hd[4], hd[5]));
            const int32_t size[2] = {prep.cols(), prep.rows()};
            fwrite(size, 4, 2, out);
            std::vector<KeyPoint> k;
            DescriptorMat d;
            prep(ext, ImageView(gray.data(), sw, sh), k, d);
            put(out, ext, k, d, size[0], size[1]);
            prep(ext, ColorImageView(colour.data(), sw, sh, 0, code), k, d);
            put(out, ext, k, d, size[0], size[1]);
            // a frame of another size than the handle's source is refused before any call
            bool threw = false;
            try {
                prep(ext, ImageView(gray.data(), sw - 1, sh), k, d);
            } catch (const std::invalid_argument&) {
                threw = true;
            }
            if (!threw) return fprintf(stderr, "a frame of the wrong size was accepted\n"), 1;
        }   // (the FrontPrep goes before the extractor whose context created it)
        std::vector<uint8_t> bm;
        ConvertMaskBirdview(bird.data(), bw, bh, 0, 3, bm);
        fwrite(bm.data(), 1, bm.size(), out);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    fclose(out);
    return rc;
}
