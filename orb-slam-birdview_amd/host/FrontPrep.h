/*
 * The mono_fisheye driver's input over liborbgpu (Examples/Monocular/mono_fisheye.cc:94-116): applyMask(im, im_masked,
 * mask_img), the crop Rect(0, 0, 1900, 800) and cv::resize(im, im, Size(0, 0), 0.5, 0.5), with the cvtColor of
 * Tracking::GrabImageMonocularWithBirdview (Tracking.cc:278-307), as one pass on the GPU; and ConvertMaskBirdview
 * (:244-271) for the birdview mask of every frame.  A FrontPrep is built once per camera from the camera mask and the
 * crop and keeps them on the GPU (orb_prep, include/orbgpu.h); its results are byte for byte the CPU definition
 * orb_front_prep_host.  GPU failures throw ORB_SLAM2::OrbGpuError.
 */
#ifndef ORBGPU_HOST_FRONTPREP_H
#define ORBGPU_HOST_FRONTPREP_H

#include <vector>

#include "ORBextractor.h"

namespace ORB_SLAM2 {

// The camera mask (cv::Mat mask_img stand-in; with OpenCV: MaskView(mask.data, mask.cols, mask.rows, mask.step,
// mask.channels())): 1 or 3 interleaved channels, rows `step` bytes apart; of a 3-channel mask channel 1 is read.
struct MaskView {
    const uint8_t* data = nullptr;
    int cols = 0, rows = 0;
    size_t step = 0;
    int channels = 3;
    MaskView() = default;
    MaskView(const uint8_t* d, int c, int r, size_t s, int ch)
        : data(d), cols(c), rows(r), step(s ? s : (size_t)c * ch), channels(ch) {}
    bool empty() const { return data == nullptr || cols <= 0 || rows <= 0; }
};

// cv::Rect stand-in
struct CropRect {
    int x = 0, y = 0, width = 0, height = 0;
    CropRect() = default;
    CropRect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

// ConvertMaskBirdview(src, dst) on the CPU (orb_bird_mask_host): src 3 or 4 interleaved channels, dst receives
// cols * rows bytes (rows packed): 0 where G < 20, else 250, the vehicle footprint zeroed.
void ConvertMaskBirdview(const uint8_t* src, int cols, int rows, size_t step, int channels, std::vector<uint8_t>& dst);

class FrontPrep {
public:
    // ctx: any context of the GPU the frames are extracted on (e.g. mpORBextractorLeft->context()); destroy the
    // FrontPrep before it.  The camera's frames are srcCols x srcRows; mask (may be empty: nothing is zeroed) has that
    // size; crop lies inside the frame and has even sides.
    FrontPrep(orb_ctx* ctx, int srcCols, int srcRows, const MaskView& mask, const CropRect& crop);
    ~FrontPrep();
    FrontPrep(const FrontPrep&) = delete;
    FrontPrep& operator=(const FrontPrep&) = delete;

    // the prepared image's size: crop.width / 2, crop.height / 2
    int cols() const { return cols_; }
    int rows() const { return rows_; }
    // what ORBextractor::operator()(frame, prep, ...) and orb_front_prep_device take
    const orb_prep* handle() const { return h_; }

    // The driver's loop body up to the keypoints: the raw frame (gray or colour) masked, cropped, halved, converted and
    // extracted on the GPU by `extractor`, whose mvImagePyramid[0] is then the prepared gray image.
    void operator()(ORBextractor& extractor, const ImageView& frame, std::vector<KeyPoint>& mvKeys,
                    DescriptorMat& mDescriptors) const;
    void operator()(ORBextractor& extractor, const ColorImageView& frame, std::vector<KeyPoint>& mvKeys,
                    DescriptorMat& mDescriptors) const;

private:
    orb_prep* h_ = nullptr;
    int cols_ = 0, rows_ = 0;
};

}  // namespace ORB_SLAM2

#endif
