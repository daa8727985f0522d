// ORB_SLAM2::Rectifier: the stereo examples' cv::remap pair over liborbgpu.
#include "Rectifier.h"

#include <stdexcept>

namespace ORB_SLAM2 {

static void check(int st, const char* what) {
    if (st != ORB_OK) throw OrbGpuError(st, what);
}

void RectifyMaps(const double K[9], const std::vector<double>& D, const double R[9], const double P33[9], int cols,
                 int rows, std::vector<float>& M1, std::vector<float>& M2) {
    if (cols < 0 || rows < 0) throw std::invalid_argument("RectifyMaps: negative size");
    M1.assign((size_t)cols * rows, 0.0f);
    M2.assign((size_t)cols * rows, 0.0f);
    check(orb_rectify_maps_host(K, D.data(), (int)D.size(), R, P33, cols, rows, M1.data(), M2.data(),
                                (size_t)cols * sizeof(float)),
          "orb_rectify_maps_host");
}

Rectifier::Rectifier(orb_ctx* ctx, const MapView& left, const MapView& right) : ctx_(ctx) {
    if (left.cols != right.cols || left.rows != right.rows)
        throw std::invalid_argument("Rectifier: the left and right maps differ in size");
    cols_ = left.cols;
    rows_ = left.rows;
    check(orb_rectify_create(ctx, left.cols, left.rows, left.x, left.y, left.step, &h_[LEFT]), "orb_rectify_create");
    const int st = orb_rectify_create(ctx, right.cols, right.rows, right.x, right.y, right.step, &h_[RIGHT]);
    if (st != ORB_OK) {
        orb_rectify_destroy(h_[LEFT]);
        throw OrbGpuError(st, "orb_rectify_create");
    }
}

Rectifier::~Rectifier() {
    orb_rectify_destroy(h_[LEFT]);
    orb_rectify_destroy(h_[RIGHT]);
}

void Rectifier::remap(Eye eye, const ImageView& im, std::vector<uint8_t>& imRect) const {
    imRect.assign((size_t)cols_ * rows_, 0);
    const bool none = im.empty();
    check(orb_remap(ctx_, h_[eye], none ? nullptr : im.data, none ? 0 : im.cols, none ? 0 : im.rows, none ? 0 : im.step,
                    imRect.data(), (size_t)cols_),
          "orb_remap");
}

void Rectifier::operator()(ORBextractor& left, ORBextractor& right, const ImageView& imLeft, const ImageView& imRight,
                           std::vector<KeyPoint>& mvKeys, DescriptorMat& mDescriptors,
                           std::vector<KeyPoint>& mvKeysRight, DescriptorMat& mDescriptorsRight) const {
    left(imLeft, h_[LEFT], ImageView(), mvKeys, mDescriptors);
    right(imRight, h_[RIGHT], ImageView(), mvKeysRight, mDescriptorsRight);
}

}  // namespace ORB_SLAM2
