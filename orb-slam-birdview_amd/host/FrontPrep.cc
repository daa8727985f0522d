// ORB_SLAM2::FrontPrep: the mono_fisheye driver's mask, crop, half-size resize and cvtColor over liborbgpu.
#include "FrontPrep.h"

#include <stdexcept>

namespace ORB_SLAM2 {

static void check(int st, const char* what) {
    if (st != ORB_OK) throw OrbGpuError(st, what);
}

void ConvertMaskBirdview(const uint8_t* src, int cols, int rows, size_t step, int channels, std::vector<uint8_t>& dst) {
    if (cols < 0 || rows < 0) throw std::invalid_argument("ConvertMaskBirdview: negative size");
    dst.assign((size_t)cols * rows, 0);
    check(orb_bird_mask_host(channels, src, cols, rows, step ? step : (size_t)cols * channels, dst.data(), (size_t)cols),
          "orb_bird_mask_host");
}

FrontPrep::FrontPrep(orb_ctx* ctx, int srcCols, int srcRows, const MaskView& mask, const CropRect& crop) {
    if (!mask.empty() && (mask.cols != srcCols || mask.rows != srcRows))
        throw std::invalid_argument("FrontPrep: the mask has not the frame's size");
    check(orb_prep_create(ctx, srcCols, srcRows, mask.empty() ? nullptr : mask.data, mask.channels, mask.step, crop.x,
                          crop.y, crop.width, crop.height, &h_),
          "orb_prep_create");
    cols_ = crop.width / 2;
    rows_ = crop.height / 2;
}

FrontPrep::~FrontPrep() { orb_prep_destroy(h_); }

void FrontPrep::operator()(ORBextractor& extractor, const ImageView& frame, std::vector<KeyPoint>& mvKeys,
                           DescriptorMat& mDescriptors) const {
    extractor(frame, h_, ImageView(), mvKeys, mDescriptors);
}

void FrontPrep::operator()(ORBextractor& extractor, const ColorImageView& frame, std::vector<KeyPoint>& mvKeys,
                           DescriptorMat& mDescriptors) const {
    extractor(frame, h_, ImageView(), mvKeys, mDescriptors);
}

}  // namespace ORB_SLAM2
