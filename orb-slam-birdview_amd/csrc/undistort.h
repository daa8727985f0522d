// cv::fisheye::undistortPoints as Frame::UndistortKeyPoints and Frame::ComputeImageBounds call it (Frame.cc:571-660:
// K = P = mK, D = mDistCoef's four floats read as k1..k4, R empty), pinned to OpenCV 3.2 fisheye.cpp on x86-64 without
// FMA.  One function for the kernel (undistort.hip) and the host twin (orb_undistort_points_host): both
// translation units are built -ffp-contract=off, and double add, multiply, divide and sqrt are correctly rounded on
// both sides, so theta is the same number on both.  tan is not: the caller passes its own (std::tan on the host, the
// definition; the device's in the kernel, which brackets it with a guard band).
#pragma once
#include <cmath>
#include <cstring>

#include "orbgpu_ctx.h"

namespace orbgpu {

// The camera widened to double once per call
struct Distortion {
    double fx, fy, cx, cy, k[4];
    int identity;   // mDistCoef.at<float>(0) == 0.0: mvKeysUn = mvKeys (Frame.cc:573)
};

inline Distortion widen(const orb_distortion& d) {
    return Distortion{(double)d.fx,   (double)d.fy,   (double)d.cx,   (double)d.cy,
                      {(double)d.k[0], (double)d.k[1], (double)d.k[2], (double)d.k[3]},
                      d.k[0] == 0.0f};
}

// What precedes the tangent: pw, theta_d (clipped) and the fixed 10 iterations of theta.  theta_d <= 1e-8 (and a NaN
// theta_d, which std::max / std::min turn into -pi/2): scale = 1, no tangent (th = 0 returned, iterate = false).
struct UndistortTheta {
    double pw0, pw1, th_d, th;
    bool iterate;
};

__host__ __device__ inline UndistortTheta undistort_theta(const Distortion& D, float x, float y) {
    UndistortTheta t;
    t.pw0 = ((double)x - D.cx) / D.fx;
    t.pw1 = ((double)y - D.cy) / D.fy;
    double th_d = sqrt(t.pw0 * t.pw0 + t.pw1 * t.pw1);
    const double half_pi = 3.1415926535897932384626433832795 / 2.0;   // CV_PI / 2
    const double lo = -half_pi;
    th_d = lo < th_d ? th_d : lo;            // std::max(-CV_PI / 2, theta_d)
    th_d = half_pi < th_d ? half_pi : th_d;  // std::min(..., CV_PI / 2)
    t.th_d = th_d;
    t.th = 0.0;
    t.iterate = th_d > 1e-8;
    if (t.iterate) {
        double th = th_d;
        for (int j = 0; j < 10; j++) {
            const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
            th = th_d / (1 + D.k[0] * t2 + D.k[1] * t4 + D.k[2] * t6 + D.k[3] * t8);
        }
        t.th = th;
    }
    return t;
}

// A float result as it is stored: every NaN as 0x7FC00000 (payload and sign differ between libms)
__host__ __device__ inline uint32_t undistort_bits(float v) {
    if (v != v) return 0x7FC00000u;
    uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = __float_as_uint(v);
#else
    std::memcpy(&b, &v, 4);
#endif
    return b;
}

// pu = pw * scale, then P * (pu, 1) with OpenCV's Matx product (sums from 0, left to right) and the division by its
// third row
__host__ __device__ inline void undistort_project(const Distortion& D, const UndistortTheta& t, double scale,
                                                  uint32_t& ox, uint32_t& oy) {
    const double pu0 = t.pw0 * scale, pu1 = t.pw1 * scale;
    const double pr0 = ((0 + D.fx * pu0) + 0 * pu1) + D.cx * 1;
    const double pr1 = ((0 + 0 * pu0) + D.fy * pu1) + D.cy * 1;
    const double pr2 = ((0 + 0 * pu0) + 0 * pu1) + 1 * 1;
    ox = undistort_bits((float)(pr0 / pr2));
    oy = undistort_bits((float)(pr1 / pr2));
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The definition: one point on the host (the bits of the two floats)
void undistort_point_host(const Distortion& D, float x, float y, uint32_t& ox, uint32_t& oy);
#endif

// The argument checks the entry points over extraction slots share (nullptr: accepted; else the reason)
const char* distortion_fault(const orb_distortion* d);
const char* grid_fault(float min_x, float min_y, float inv_w, float inv_h);   // orb_frame_create's grid checks
const char* batch_fault(int nframes, int kp_cap);

// The step that gives a batch its mvuRight / mvDepth, between the undistort step and the grids:
//   kRgbd    Frame::ComputeStereoFromRGBD (rgbd.hip) over the depth maps `map` (device memory) and mbf;
//   kStereo  Frame::ComputeStereoMatches (stereo.hip) with mb and mbf: the batch then holds (left, right) slot pairs,
//            frame p of the call is slot 2 p, and the search reads the images and pyramids of the context's last batch.
// mvuRight / mvDepth go to d_uright / d_depth (nframes * kp_cap floats each; nullptr: working space).
struct DepthStep {
    enum Kind { kRgbd, kStereo } kind;
    orb_depth_map map;   // kRgbd
    float mb;            // kStereo
    float mbf;
    float* d_uright;
    float* d_depth;
    int slots() const { return kind == kStereo ? 2 : 1; }   // batch slots per frame
};

// The creators of resident frames from extraction slots: orb_frame_create_from_extract (d_counts nullptr, one frame of
// n_single keypoints, d_uright optional), orb_frames_create_from_batch and, with a step,
// orb_frames_create_from_batch_rgbd / _stereo (every handle's uright is then the step's).  Arguments are checked by the
// caller.
int frames_from_extract(const char* fn, Ctx* c, const orb_distortion* dist, int nframes, const uint8_t* d_desc,
                        const orb_keypoint* d_raw, const int* d_counts, int n_single, int kp_cap, const float* d_uright,
                        float min_x, float min_y, float inv_w, float inv_h, orb_frame** out,
                        const DepthStep* step = nullptr);

}  // namespace orbgpu
