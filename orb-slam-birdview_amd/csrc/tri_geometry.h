// SearchForTriangulation's pair-dependent float work, in the reference build's contracted forms
// (tools/ref_flags_probe.cpp), compiled by the host (tri_geometry_body, matcher.hip: the staged records of
// k_triangulation) and by the device (k_triangulation_frames, hamming_kernels.hip: resident frames; the distance test
// of both kernels): one definition of each form.  Every fma is exact whether it is an instruction or libm's fmaf; the translation units that include
// this build with -ffp-contract=off, so the fmaf below are the only fused operations.
#pragma once

#if defined(__HIPCC__)
#define ORB_TRI_HD __host__ __device__
#else
#define ORB_TRI_HD
#endif

namespace orbgpu {

// CheckDistEpipolarLine's line of the KF1 keypoint (x, y) in KF2 (ORBmatcher.cc:143-145), F row-major 3x3:
// a = fma(x, F00, y F10) + F20, b likewise, c = fma(y, F12, x F02) + F22.
__attribute__((always_inline)) ORB_TRI_HD inline void tri_line(float x, float y, const float* F, float& a, float& b,
                                                               float& c) {
    a = __builtin_fmaf(x, F[0], y * F[3]) + F[6];
    b = __builtin_fmaf(x, F[1], y * F[4]) + F[7];
    c = __builtin_fmaf(y, F[5], x * F[2]) + F[8];
}

// The epipole gate of a KF2 keypoint (x, y) of octave oct (:743-748): inside the radius iff
// fma(dex, dex, dey dey) < 100 scale2[oct].
__attribute__((always_inline)) ORB_TRI_HD inline bool tri_near_epipole(float ex, float ey, float x, float y,
                                                                       const float* scale2, int oct) {
    const float dex = ex - x, dey = ey - y;
    return __builtin_fmaf(dex, dex, dey * dey) < 100 * scale2[oct];
}

// pKF2->mvLevelSigma2[kp2.octave] (:156)
__attribute__((always_inline)) ORB_TRI_HD inline float tri_sigma2(const float* sigma2, int oct) { return sigma2[oct]; }

// CheckDistEpipolarLine's distance test of a KF2 keypoint (x, y) against the line a, b, c (:147-156), den =
// fma(a, a, b b) computed once per line: den == 0 refuses; num = fma(b, y, a x) + c, dsqr = num num / den in float, and
// the compare dsqr < 3.84 sigma2 in double (a NaN refuses).  Device only in use: both triangulation kernels call it,
// and the host has no copy of this test.
__attribute__((always_inline)) ORB_TRI_HD inline bool tri_epipolar_ok(float la, float lb, float lc, float den, float x,
                                                                      float y, float sigma2) {
    if (den == 0) return false;
    const float num = __builtin_fmaf(lb, y, la * x) + lc;
    const float dsqr = num * num / den;
    return (double)dsqr < 3.84 * (double)sigma2;
}

}  // namespace orbgpu
