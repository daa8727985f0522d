/*
 * Frame::ComputeStereoMatches (src/Frame.cc:662-836) over liborbgpu: the stereo consumer of the
 * extractor's outputs.  The reference method reads mvKeys / mDescriptors / mvKeysRight /
 * mDescriptorsRight, the two extractors' mvImagePyramid, mb and mbf, and writes mvuRight / mvDepth;
 * this mirror takes exactly those members.  The window search reads the pyramids where the GPU
 * extraction left them (no mvImagePyramid download).  Both extractors must sit on one device and
 * have extracted the left / right image last.  GPU failures throw ORB_SLAM2::OrbGpuError.
 */
#ifndef ORBGPU_HOST_STEREO_H
#define ORBGPU_HOST_STEREO_H

#include <vector>

#include "ORBextractor.h"

namespace ORB_SLAM2 {

// Returns the number of left keypoints that received a depth.
int ComputeStereoMatches(const ORBextractor& left, const ORBextractor& right, const std::vector<KeyPoint>& mvKeys,
                         const DescriptorMat& mDescriptors, const std::vector<KeyPoint>& mvKeysRight,
                         const DescriptorMat& mDescriptorsRight, float mb, float mbf, std::vector<float>& mvuRight,
                         std::vector<float>& mvDepth);

// Frame::ComputeStereoFromRGBD (src/Frame.cc:839-860) with Tracking::GrabImageRGBD's convertTo folded in
// (Tracking.cc:229-230): imDepth is the RAW depth image (CV_16U or CV_32F as orb_depth_map names them, host memory)
// with factor = mDepthMapFactor; mvKeys gives the pixel, mvKeysUn the x of mvuRight.  Runs on the CPU (one frame's
// keypoints are on the host already: orb_stereo_from_rgbd_host is the definition and the right call).  Returns the
// number of keypoints with a depth; a keypoint outside the image throws OrbGpuError (the reference reads outside it).
int ComputeStereoFromRGBD(const orb_depth_map& imDepth, const std::vector<KeyPoint>& mvKeys,
                          const std::vector<KeyPoint>& mvKeysUn, float mbf, std::vector<float>& mvuRight,
                          std::vector<float>& mvDepth);

}  // namespace ORB_SLAM2

#endif
