/*
 * The stereo examples' rectification over liborbgpu: cv::remap(imLeft, imLeftRect, M1l, M2l, cv::INTER_LINEAR) and the
 * same for the right eye (Examples/Stereo/stereo_euroc.cc:136-137, Examples/ROS/ORB_SLAM2/src/ros_stereo.cc:161-162).
 * A Rectifier is built once per stereo rig from the four CV_32FC1 maps of cv::initUndistortRectifyMap (:97-98) and
 * keeps them on the GPU in fixed point (orb_rectify, include/orbgpu.h); its results are byte for byte OpenCV 3.2's
 * remap for 8-bit one-channel images (the CPU definition is orb_remap_host).  Without OpenCV the maps come from
 * RectifyMaps below (orb_rectify_maps_host).  GPU failures throw ORB_SLAM2::OrbGpuError.
 */
#ifndef ORBGPU_HOST_RECTIFIER_H
#define ORBGPU_HOST_RECTIFIER_H

#include <vector>

#include "ORBextractor.h"

namespace ORB_SLAM2 {

// A CV_32FC1 map pair (cv::Mat M1, M2 stand-in; with OpenCV: MapView((const float*)M1.data, (const float*)M2.data,
// M1.cols, M1.rows, M1.step)): rows `step` bytes apart.
struct MapView {
    const float* x = nullptr;
    const float* y = nullptr;
    int cols = 0, rows = 0;
    size_t step = 0;
    MapView() = default;
    MapView(const float* x_, const float* y_, int c, int r, size_t s = 0)
        : x(x_), y(y_), cols(c), rows(r), step(s ? s : (size_t)c * sizeof(float)) {}
};

// cv::initUndistortRectifyMap(K, D, R, P.rowRange(0, 3).colRange(0, 3), cv::Size(cols, rows), CV_32F, M1, M2) on the CPU:
// K, R, P33 nine doubles row-major, D 4, 5 or 8 coefficients.  M1 / M2 receive cols * rows floats each.
void RectifyMaps(const double K[9], const std::vector<double>& D, const double R[9], const double P33[9], int cols,
                 int rows, std::vector<float>& M1, std::vector<float>& M2);

class Rectifier {
public:
    enum Eye { LEFT = 0, RIGHT = 1 };

    // ctx: any context of the GPU the images are extracted on (e.g. mpORBextractorLeft->context()); destroy the
    // Rectifier before it.  The two map pairs have one size, which is the rectified images'.
    Rectifier(orb_ctx* ctx, const MapView& left, const MapView& right);
    ~Rectifier();
    Rectifier(const Rectifier&) = delete;
    Rectifier& operator=(const Rectifier&) = delete;

    int cols() const { return cols_; }
    int rows() const { return rows_; }
    // one eye's resident map: what ORBextractor::operator()(rawImage, rectify, ...) and orb_remap_device take
    const orb_rectify* handle(Eye eye) const { return h_[eye]; }
    // both, in the order of the interleaved left / right batch layout (orb_remap_device with nmaps = 2)
    const orb_rectify* const* handles() const { return h_; }

    // cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) of one eye on the GPU: imRect receives cols() * rows() bytes
    // (rows packed).  An empty image gives an all-zero imRect (every tap is outside).
    void remap(Eye eye, const ImageView& im, std::vector<uint8_t>& imRect) const;

    // The stereo examples' loop body up to the keypoints: both raw images rectified and extracted on the GPU, the left
    // by `left`, the right by `right` (mpORBextractorLeft / Right), which are then valid arguments of
    // ComputeStereoMatches (host/Stereo.h).
    void operator()(ORBextractor& left, ORBextractor& right, const ImageView& imLeft, const ImageView& imRight,
                    std::vector<KeyPoint>& mvKeys, DescriptorMat& mDescriptors, std::vector<KeyPoint>& mvKeysRight,
                    DescriptorMat& mDescriptorsRight) const;

private:
    orb_ctx* ctx_ = nullptr;
    orb_rectify* h_[2] = {nullptr, nullptr};
    int cols_ = 0, rows_ = 0;
};

}  // namespace ORB_SLAM2

#endif
