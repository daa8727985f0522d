// Birdview ORB stream of Frame::Frame (reference src/Frame.cc:318-342) on gfx950 — SURVEY §8(f) row 3.
//
// The reference runs OpenCV's own cv::ORB (not ORBextractor) on the birdview image:
//     mask = birdviewMask with the vehicle footprint zeroed          Frame.cc:320-327
//     cv::ORB::create(2000)->detect(img, kps, mask)                  Frame.cc:329-330
//     cv::cornerSubPix(img, pts, (5,5), (-1,-1), EPS|ITER 40 0.001)  Frame.cc:331-341
//     cv::ORB::compute(img, kps, desc)                               Frame.cc:342
// restated from OpenCV 3.2 orb.cpp / keypoint.cpp / cornersubpix.cpp / samplers.cpp (the oracle's
// oracle/cvorb_oracle.inc states each detail).
//
// Every kernel carries a frame dimension: the single-frame calls run it with one frame, the batch calls
// (orb_bird_extract_batch*) run each stage once for up to ORB_BIRD_MAX_BATCH frames of one size.
// Device side: pyramid (+ mask pyramid) by per-level resize launches, one FAST score-map launch over
// all levels, a count / scan / emit pass that writes the masked, border-filtered, non-max-suppressed
// candidates of every level in raster order together with their Harris responses, the 7x7 blurred
// pyramid, and per-keypoint IC angle, cornerSubPix and rBRIEF kernels.
// Host side: KeyPointsFilter::retainBest (std::nth_element + std::partition) — the reference's own
// sequential selection, whose output ORDER is libstdc++'s introselect order, so it runs on the host
// with the same library call the OpenCV build makes.
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "glibc_trig.h"
#include "orbgpu_ctx.h"

namespace orbgpu {
namespace {

constexpr int kBirdMaxLevels = ORBGPU_MAX_LEVELS;
constexpr int kSubWin = 5;                     // cornerSubPix win (5,5): 11 x 11 window, 13 x 13 patch
constexpr int kSubW = 2 * kSubWin + 1;
constexpr int kSubP = kSubW + 2;

struct BirdLevel {
    int w, h, pitch;
    int pad;
    long long off;     // byte offset of the level in a pyramid buffer
    float scale;       // getScale(level) = (float)pow(scaleFactor, level)
    int nfeat;         // nfeaturesPerLevel
};

struct BirdGeom {
    int nlevels, W, H, edge, fastTh;
    int variant;           // ORB_VARIANT_RESIZE_GENERIC / ORB_VARIANT_BLUR_HALFUP (orb_bird_params.variant)
    float harris_scale4;   // (1 / (4 * 7 * 255.f))^4
    int gk[8];             // 7-tap Gaussian sigma 2, 8-bit fixed point
    int umax[16];          // orb.cpp computeKeyPoints u_max (halfPatchSize 15)
    BirdLevel L[kBirdMaxLevels];
};

// candidate record of the emit pass
struct BirdCand {
    int xy;          // x | y << 16 (level coordinates)
    int level;
    int score;       // FAST score (KeyPoint::response before Harris)
    float harris;    // HarrisResponses(blockSize 7, k 0.04)
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int reflect101_d(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

/* ---------------- pyramid: cv::resize(prev level, INTER_LINEAR) (orb.cpp detectAndCompute) --------
 * blockIdx.z < nframes is that frame's image pyramid; blockIdx.z - nframes is a mask pyramid (one when
 * the batch shares its mask, one per frame otherwise): resize of the previous (thresholded) mask level,
 * then threshold(254, 0, THRESH_TOZERO).  fpitch: bytes between two frames' pyramids. */
__global__ __launch_bounds__(256) void k_bird_resize(const BirdGeom* __restrict__ g, int l,
                                                     const ResizeCoef* __restrict__ coef, uint8_t* __restrict__ pyr,
                                                     uint8_t* __restrict__ mpyr, int nframes, unsigned fpitch) {
    const BirdLevel D = g->L[l], S = g->L[l - 1];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= D.w) return;
    const bool is_mask = (int)blockIdx.z >= nframes;
    uint8_t* base = is_mask ? mpyr + (size_t)(blockIdx.z - nframes) * fpitch : pyr + (size_t)blockIdx.z * fpitch;
    const ResizeCoef cx = coef[x], cy = coef[D.w + y];
    const uint8_t* r0 = base + S.off + (long long)cy.s0 * S.pitch;
    const uint8_t* r1 = base + S.off + (long long)cy.s1 * S.pitch;
    const int h0 = r0[cx.s0] * cx.c0 + r0[cx.s1] * cx.c1;
    const int h1 = r1[cx.s0] * cx.c0 + r1[cx.s1] * cx.c1;
    int v = (g->variant & ORB_VARIANT_RESIZE_GENERIC)
                ? min((cy.c0 * h0 + cy.c1 * h1 + (1 << 21)) >> 22, 255)   // generic FixedPtCast
                : (((cy.c0 * (h0 >> 4)) >> 16) + ((cy.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
    if (is_mask) v = v > 254 ? v : 0;
    base[D.off + (long long)y * D.pitch + x] = (uint8_t)v;
}

/* ---------------- level 0 of a device-resident batch ----------------------------------------------------
 * blockIdx.z < nframes copies frame z into its pyramid's level 0; blockIdx.z - nframes copies a mask and
 * zeroes the vehicle footprint [fx0, fx1) x [fy0, fy1) in the copy (Frame.cc:320-327), so the caller's
 * mask is only read. */
__global__ __launch_bounds__(256) void k_bird_ingest(const BirdGeom* __restrict__ g, const uint8_t* __restrict__ imgs,
                                                     size_t stride, size_t frame_pitch,
                                                     const uint8_t* __restrict__ masks, size_t mstride,
                                                     size_t mask_frame_pitch, uint8_t* __restrict__ pyr,
                                                     uint8_t* __restrict__ mpyr, int nframes, unsigned fpitch, int fx0,
                                                     int fy0, int fx1, int fy1) {
    const BirdLevel L = g->L[0];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= L.w) return;
    const unsigned d = (unsigned)L.off + y * L.pitch + x;
    if ((int)blockIdx.z < nframes) {
        (pyr + (size_t)blockIdx.z * fpitch)[d] = (imgs + blockIdx.z * frame_pitch)[y * stride + x];
    } else {
        const unsigned m = blockIdx.z - nframes;
        const bool foot = fx0 <= x && x < fx1 && fy0 <= y && y < fy1;
        (mpyr + (size_t)m * fpitch)[d] = foot ? (uint8_t)0 : (masks + m * mask_frame_pitch)[y * mstride + x];
    }
}

/* ---------------- FAST 9/16 score map (cv::FAST, threshold fastThreshold, TYPE_9_16) -------------
 * score = (max over 9-arcs of the arc's weakest |v - p|, same sign) - 1 when that exceeds the
 * threshold (OpenCV cornerScore<16>), else 0.  Only rows/columns [edge-1, dim-edge] are scored: every
 * candidate that survives runByImageBorder(edge) lies in [edge, dim-edge) and its NMS neighbours one
 * pixel further out.  rows: (level, y) table; blockIdx.z: frame. */
__device__ __forceinline__ int fast_score_at(const uint8_t* c, int P, int t) {
    const int v = c[0];
    int d[16];
    d[0] = v - c[3 * P];
    d[1] = v - c[1 + 3 * P];
    d[2] = v - c[2 + 2 * P];
    d[3] = v - c[3 + 1 * P];
    d[4] = v - c[3];
    d[5] = v - c[3 - 1 * P];
    d[6] = v - c[2 - 2 * P];
    d[7] = v - c[1 - 3 * P];
    d[8] = v - c[-3 * P];
    d[9] = v - c[-1 - 3 * P];
    d[10] = v - c[-2 - 2 * P];
    d[11] = v - c[-3 - 1 * P];
    d[12] = v - c[-3];
    d[13] = v - c[-3 + 1 * P];
    d[14] = v - c[-2 + 2 * P];
    d[15] = v - c[-1 + 3 * P];
    int m3[16], x3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        m3[k] = min(min(d[k], d[(k + 1) & 15]), d[(k + 2) & 15]);
        x3[k] = max(max(d[k], d[(k + 1) & 15]), d[(k + 2) & 15]);
    }
    int A = 0, Bn = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        A = max(A, min(min(m3[k], m3[(k + 3) & 15]), m3[(k + 6) & 15]));
        Bn = min(Bn, max(max(x3[k], x3[(k + 3) & 15]), x3[(k + 6) & 15]));
    }
    const int s = max(A, -Bn);
    return s > t ? s - 1 : 0;
}

__global__ __launch_bounds__(256) void k_bird_fast(const BirdGeom* __restrict__ g, const int2* __restrict__ rows,
                                                   const uint8_t* __restrict__ pyr, uint8_t* __restrict__ score,
                                                   unsigned fpitch) {
    const int2 r = rows[blockIdx.y];
    const BirdLevel L = g->L[r.x];
    const int x = g->edge - 1 + blockIdx.x * 256 + threadIdx.x;
    if (x > L.w - g->edge) return;
    pyr += (size_t)blockIdx.z * fpitch;
    score += (size_t)blockIdx.z * fpitch;
    const long long o = L.off + (long long)r.y * L.pitch + x;
    const uint8_t* c = pyr + o;
    const int P = L.pitch, t = g->fastTh, v = c[0];
    // compass prefilter (a 9-arc holds two cyclically adjacent compass points): necessary for a corner
    const int p0 = c[3 * P], p4 = c[3], p8 = c[-3 * P], p12 = c[-3];
    const int hi = v + t, lo = v - t;
    const int bm = (p0 > hi) | ((p4 > hi) << 1) | ((p8 > hi) << 2) | ((p12 > hi) << 3);
    const int dm = (p0 < lo) | ((p4 < lo) << 1) | ((p8 < lo) << 2) | ((p12 < lo) << 3);
    score[o] = ((0xFAC8 >> bm) | (0xFAC8 >> dm)) & 1 ? (uint8_t)fast_score_at(c, P, t) : (uint8_t)0;
}

/* ---------------- candidates: NMS + runByPixelsMask + runByImageBorder, raster order ------------
 * One wave per (level, y) row of [edge, h-edge) of frame blockIdx.y; mode 0 counts, mode 1 writes at
 * the scanned offsets of the frame's candidate slot with the Harris response (orb.cpp HarrisResponses, blockSize 7, HARRIS_K 0.04f: integer
 * gradient sums, then the float formula in the reference's evaluation order). */
template <int kMode>
__global__ __launch_bounds__(256) void k_bird_cands(const BirdGeom* __restrict__ g, const int2* __restrict__ rows,
                                                    int nrows, const uint8_t* __restrict__ pyr,
                                                    const uint8_t* __restrict__ mpyr, const uint8_t* __restrict__ score,
                                                    int* __restrict__ rowcnt, const int* __restrict__ rowoff,
                                                    BirdCand* __restrict__ out, unsigned fpitch, unsigned mfpitch,
                                                    unsigned cand_slot) {
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= nrows) return;
    {   // this frame's pyramid, mask pyramid (mfpitch 0: shared), score map, row tables and candidate slot
        const unsigned f = blockIdx.y;
        pyr += (size_t)f * fpitch;
        score += (size_t)f * fpitch;
        if (mpyr) mpyr += (size_t)f * mfpitch;
        if (kMode) {
            rowoff += f * (nrows + 1);
            out += (size_t)f * cand_slot;
        } else {
            rowcnt += f * (nrows + 1);
        }
    }
    const int2 r = rows[wid];
    const BirdLevel L = g->L[r.x];
    const int e = g->edge, P = L.pitch;
    int pos = kMode ? rowoff[wid] : 0;
    for (int x0 = e; x0 < L.w - e; x0 += 64) {
        const int x = x0 + lane;
        bool keep = false;
        int s = 0;
        const long long o = L.off + (long long)r.y * P + x;
        if (x < L.w - e) {
            s = score[o];
            if (s) {
                const uint8_t* q = score + o;
                keep = s > q[-1] && s > q[1] && s > q[-P - 1] && s > q[-P] && s > q[-P + 1] && s > q[P - 1] &&
                       s > q[P] && s > q[P + 1];
                if (keep && mpyr) keep = mpyr[o] != 0;
            }
        }
        const unsigned long long m = __ballot(keep);
        if (kMode) {
            // Harris responses, one candidate at a time over the whole wave: lane q < 49 takes pixel
            // (q / 7, q % 7) of the 7x7 block, the integer sums are wave reductions (order-free)
            float hr = 0.f;
            unsigned long long mm = m;
            while (mm) {
                const int src = __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                const long long oc = o - lane + src;   // the candidate's pixel (same row, x0 + src)
                int ixx = 0, iyy = 0, ixy = 0;
                if (lane < 49) {
                    const int i = lane / 7, j = lane - 7 * (lane / 7);
                    const uint8_t* q = pyr + oc + (long long)(i - 3) * P + (j - 3);
                    const int Ix = (q[1] - q[-1]) * 2 + (q[-P + 1] - q[-P - 1]) + (q[P + 1] - q[P - 1]);
                    const int Iy = (q[P] - q[-P]) * 2 + (q[P - 1] - q[-P - 1]) + (q[P + 1] - q[-P + 1]);
                    ixx = Ix * Ix;
                    iyy = Iy * Iy;
                    ixy = Ix * Iy;
                }
#pragma unroll
                for (int sft = 32; sft > 0; sft >>= 1) {
                    ixx += __shfl_xor(ixx, sft);
                    iyy += __shfl_xor(iyy, sft);
                    ixy += __shfl_xor(ixy, sft);
                }
                const float fa = (float)ixx, fb = (float)iyy, fc = (float)ixy;
                const float h = (fa * fb - fc * fc - 0.04f * (fa + fb) * (fa + fb)) * g->harris_scale4;
                if (lane == src) hr = h;
            }
            if (keep) {
                const int rank = __popcll(m & ((1ull << lane) - 1));
                BirdCand c;
                c.xy = x | (r.y << 16);
                c.level = r.x;
                c.score = s;
                c.harris = hr;
                out[pos + rank] = c;
            }
        }
        pos += __popcll(m);
    }
    if (!kMode && lane == 0) rowcnt[wid] = pos;
}

// exclusive scan of a frame's row counts (one block per frame); per-level counts from the level row ranges
__global__ __launch_bounds__(1024) void k_bird_scan(const int* __restrict__ rowcnt, int nrows,
                                                    const int* __restrict__ lvl_row0, int nlevels,
                                                    int* __restrict__ rowoff, int* __restrict__ lvlcnt) {
    __shared__ int s_w[16];
    __shared__ int s_carry;
    rowcnt += blockIdx.x * (nrows + 1);
    rowoff += blockIdx.x * (nrows + 1);
    lvlcnt += blockIdx.x * kBirdMaxLevels;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int base = 0; base < nrows; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nrows ? rowcnt[i] : 0;
        int x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_w[wv] = x;
        __syncthreads();
        int pre = 0;
        for (int k = 0; k < wv; k++) pre += s_w[k];
        const int carry = s_carry;
        if (i < nrows) rowoff[i] = carry + pre + x - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + pre + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) rowoff[nrows] = s_carry;
    __syncthreads();
    if ((int)threadIdx.x < nlevels) lvlcnt[threadIdx.x] = rowoff[lvl_row0[threadIdx.x + 1]] - rowoff[lvl_row0[threadIdx.x]];
}

/* ---------------- GaussianBlur(7x7, sigma 2, REFLECT_101) of every level ROI ----------------------
 * Integer separable filter; the column pass rounds half-to-even on columns x < (w & ~3) (OpenCV's SSE2
 * SymmColumnVec_32s8u) and half-up on the tail (FixedPtCastEx) — the oracle's gauss7_blur. */
__global__ __launch_bounds__(256) void k_bird_blur(const BirdGeom* __restrict__ g, const int2* __restrict__ rows,
                                                   const uint8_t* __restrict__ pyr, uint8_t* __restrict__ blur,
                                                   unsigned fpitch) {
    const int2 r = rows[blockIdx.y];
    const BirdLevel L = g->L[r.x];
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= L.w) return;
    blur += (size_t)blockIdx.z * fpitch;
    const uint8_t* src = pyr + (size_t)blockIdx.z * fpitch + L.off;
    int xs[7];
#pragma unroll
    for (int j = 0; j < 7; j++) xs[j] = reflect101_d(x + j - 3, L.w);
    int S = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const uint8_t* row = src + (long long)reflect101_d(r.y + i - 3, L.h) * L.pitch;
        int acc = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) acc += g->gk[j] * row[xs[j]];
        S += g->gk[i] * acc;
    }
    const int q = S >> 16, rem = S & 0xFFFF;
    int v;
    // ORB_VARIANT_BLUR_HALFUP: half-up everywhere (no SSE2 body)
    if (x < ((g->variant & ORB_VARIANT_BLUR_HALFUP) ? 0 : (L.w & ~3))) v = rem > 32768 ? q + 1 : (rem < 32768 ? q : q + (q & 1));
    else v = (S + 32768) >> 16;
    blur[L.off + (long long)r.y * L.pitch + x] = (uint8_t)min(max(v, 0), 255);
}

/* ---------------- ICAngles + pt *= layerScale (orb.cpp computeKeyPoints tail) ----------------------
 * One wave per keypoint: lane v in [0, 31) sums row v-15 of the circular patch (integer moments,
 * order-free), then cv::fastAtan2.  kframe (batch only): the frame whose pyramid keypoint k reads. */
constexpr float kAtanScale = (float)(180 / 3.14159265358979323846);
constexpr float kP1 = 0.9997878412794807f * kAtanScale;
constexpr float kP3 = -0.3258083974640975f * kAtanScale;
constexpr float kP5 = 0.1555786518463281f * kAtanScale;
constexpr float kP7 = -0.04432655554792128f * kAtanScale;
constexpr float kFactorPI = (float)(3.14159265358979323846 / 180.f);

__device__ __forceinline__ float cv_fast_atan2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)2.220446049250313e-16);
        c2 = c * c;
        a = (((kP7 * c2 + kP5) * c2 + kP3) * c2 + kP1) * c;
    } else {
        c = ax / (ay + (float)2.220446049250313e-16);
        c2 = c * c;
        a = 90.f - (((kP7 * c2 + kP5) * c2 + kP3) * c2 + kP1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

__global__ __launch_bounds__(256) void k_bird_angle(const BirdGeom* __restrict__ g, const uint8_t* __restrict__ pyr,
                                                    orb_keypoint* __restrict__ kps, int n,
                                                    const int* __restrict__ kframe, unsigned fpitch) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= n) return;
    orb_keypoint kp = kps[k];
    const BirdLevel L = g->L[kp.octave];
    if (kframe) pyr += (size_t)kframe[k] * fpitch;
    const uint8_t* center = pyr + L.off + (long long)(int)rintf(kp.y) * L.pitch + (int)rintf(kp.x);
    int m10 = 0, m01 = 0;
    if (lane < 31) {
        const int v = lane - 15, av = v < 0 ? -v : v;
        const int d = g->umax[av];
        const uint8_t* row = center + v * L.pitch;
        int sum = 0, mom = 0;
        for (int u = -d; u <= d; u++) {
            const int val = row[u];
            sum += val;
            mom += u * val;
        }
        m10 = mom;
        m01 = v * sum;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m10 += __shfl_xor(m10, o);
        m01 += __shfl_xor(m01, o);
    }
    if (lane == 0) {
        kp.angle = cv_fast_atan2((float)m01, (float)m10);
        kp.x = kp.x * L.scale;
        kp.y = kp.y * L.scale;
        kps[k] = kp;
    }
}

/* ---------------- cv::cornerSubPix(win (5,5), zeroZone (-1,-1)) --------------------------------------
 * One wavefront per point.  Per iteration: lanes 0..12 generate the 13 rows of the getRectSubPix_8u32f
 * patch (each row is a 13-step float recurrence) into LDS; lanes then compute the 121 per-pixel terms
 * (gxx, gxy, gyy, gxx*px + gxy*py, gxy*px + gyy*py, in double) into LDS; lanes 0..4 each run ONE of the
 * five accumulations sequentially in the reference's (i, j) order, so every double sum is bit-identical
 * to the sequential code; the sums are broadcast and every lane updates the point identically. */
struct SubpixSrc {
    const uint8_t* img;
    int pitch, W, H;
};

constexpr int kSubE = kSubW * kSubW;   // 121 window pixels

// one patch row r of getRectSubPix(img, (13, 13), (cx, cy)) into out[13]; interior windows read the
// point's cached neighbourhood (`cache`, pitch kSubC, origin (cx0, cy0)) when they lie inside it
constexpr int kSubC = 32;
__device__ __forceinline__ void subpix_row(const SubpixSrc& s, bool inside, int ipx, int ipy, float a, float b,
                                           double sd, int r, float (&out)[kSubP], const uint8_t* cache, int cx0,
                                           int cy0) {
    if (inside) {
        const float a12 = a * (1.f - b), a22 = a * b, b1 = 1.f - b, b2 = b;
        const bool cached = cache && ipx >= cx0 && ipx + kSubP < cx0 + kSubC && ipy >= cy0 &&
                            ipy + kSubP < cy0 + kSubC;
        const uint8_t* s0 = cached ? cache + (ipy + r - cy0) * kSubC + (ipx - cx0)
                                   : s.img + (long long)(ipy + r) * s.pitch + ipx;
        const uint8_t* s1 = s0 + (cached ? kSubC : s.pitch);
        float prev = (1 - a) * (b1 * s0[0] + b2 * s1[0]);
#pragma unroll
        for (int j = 0; j < kSubP; j++) {
            const float t = a12 * s0[j + 1] + a22 * s1[j + 1];
            out[j] = prev + t;
            prev = (float)(t * sd);
        }
    } else {
        const float a11 = (1.f - a) * (1.f - b), a12 = a * (1.f - b), a21 = (1.f - a) * b, a22 = a * b;
        const int y0 = min(max(ipy + r, 0), s.H - 1), y1 = min(max(ipy + r + 1, 0), s.H - 1);
        const uint8_t* s0 = s.img + (long long)y0 * s.pitch;
        const uint8_t* s1 = s.img + (long long)y1 * s.pitch;
#pragma unroll
        for (int j = 0; j < kSubP; j++) {
            const int x0 = min(max(ipx + j, 0), s.W - 1), x1 = min(max(ipx + j + 1, 0), s.W - 1);
            out[j] = (float)s0[x0] * a11 + (float)s0[x1] * a12 + (float)s1[x0] * a21 + (float)s1[x1] * a22;
        }
    }
}

__global__ __launch_bounds__(256) void k_bird_subpix(SubpixSrc s, const float* __restrict__ wmask, float* pts,
                                                     int stride, int n, int max_iters, double eps2, int edge,
                                                     int* __restrict__ keep, const int* __restrict__ kframe,
                                                     unsigned fpitch) {
    __shared__ float s_patch[4][kSubP * kSubP + 3];
    __shared__ double s_terms[4][5 * kSubE + 1];
    __shared__ __attribute__((aligned(16))) uint8_t s_cache[4][kSubC * kSubC];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + wv;
    if (k >= n) return;
    if (kframe) s.img += (size_t)kframe[k] * fpitch;   // batch: the level-0 image of the point's frame
    float* patch = s_patch[wv];
    double* terms = s_terms[wv];
    float* pt = pts + (long long)k * stride;
    const float cTx = pt[0], cTy = pt[1];
    // the 32 x 32 neighbourhood of the start point, staged once (windows within +-9 px of it read LDS)
    const int cx0 = (int)floorf(cTx) - 15, cy0 = (int)floorf(cTy) - 15;
    const uint8_t* cache = nullptr;
    if (cx0 >= 0 && cy0 >= 0 && cx0 + kSubC <= s.W && cy0 + kSubC <= s.H && (cTx == cTx) && (cTy == cTy)) {
        uint8_t* c = s_cache[wv];
#pragma unroll
        for (int q = 0; q < kSubC * kSubC / 64 / 4; q++) {   // 4 bytes per lane per step
            const int i = (q * 64 + lane) * 4, yy = i / kSubC, xx = i - yy * kSubC;
            const uint8_t* src = s.img + (long long)(cy0 + yy) * s.pitch + cx0 + xx;
            c[i] = src[0];
            c[i + 1] = src[1];
            c[i + 2] = src[2];
            c[i + 3] = src[3];
        }
        cache = c;
        wave_lds_sync();
    }
    float cIx = cTx, cIy = cTy;
    int iter = 0;
    double err = 0;
    do {
        const float centx = cIx - (kSubP - 1) * 0.5f, centy = cIy - (kSubP - 1) * 0.5f;
        const int ipx = (int)floorf(centx), ipy = (int)floorf(centy);
        const bool inside = 0 <= ipx && ipx + kSubP < s.W && 0 <= ipy && ipy + kSubP < s.H;
        float fa = centx - ipx, fb = centy - ipy;
        double sd = 0;
        if (inside) {
            fa = fmaxf(fa, 0.0001f);
            sd = (1. - fa) / fa;
        }
        if (lane < kSubP) {
            float row[kSubP];
            subpix_row(s, inside, ipx, ipy, fa, fb, sd, lane, row, cache, cx0, cy0);
#pragma unroll
            for (int j = 0; j < kSubP; j++) patch[lane * kSubP + j] = row[j];
        }
        wave_lds_sync();
        for (int e = lane; e < kSubE; e += 64) {
            const int i = e / kSubW, j = e - i * kSubW;
            const float* sp = patch + (i + 1) * kSubP + (j + 1);
            const double m = wmask[e];
            const double tgx = sp[1] - sp[-1];
            const double tgy = sp[kSubP] - sp[-kSubP];
            const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
            const double px = j - kSubWin, py = i - kSubWin;
            terms[e] = gxx;
            terms[kSubE + e] = gxy;
            terms[2 * kSubE + e] = gyy;
            terms[3 * kSubE + e] = gxx * px + gxy * py;
            terms[4 * kSubE + e] = gxy * px + gyy * py;
        }
        wave_lds_sync();
        double acc = 0;
        if (lane < 5) {   // in order; row g+1's loads are in flight while row g is added
            const double* t = terms + lane * kSubE;
            double v[kSubW], w[kSubW];
#pragma unroll
            for (int j = 0; j < kSubW; j++) v[j] = t[j];
#pragma unroll
            for (int g = 0; g < kSubW; g++) {
                if (g + 1 < kSubW) {
#pragma unroll
                    for (int j = 0; j < kSubW; j++) w[j] = t[(g + 1) * kSubW + j];
                }
#pragma unroll
                for (int j = 0; j < kSubW; j++) acc += v[j];
#pragma unroll
                for (int j = 0; j < kSubW; j++) v[j] = w[j];
            }
        }
        const double a = __shfl(acc, 0), b = __shfl(acc, 1), c = __shfl(acc, 2), bb1 = __shfl(acc, 3),
                     bb2 = __shfl(acc, 4);
        wave_lds_sync();   // this iteration's LDS reads precede the next iteration's patch stores
        const double det = a * c - b * b;
        if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) break;
        const double sc = 1.0 / det;
        const float nx = (float)(cIx + c * sc * bb1 - b * sc * bb2);
        const float ny = (float)(cIy - b * sc * bb1 + a * sc * bb2);
        err = (nx - cIx) * (nx - cIx) + (ny - cIy) * (ny - cIy);
        cIx = nx;
        cIy = ny;
        if (cIx < 0 || cIx >= s.W || cIy < 0 || cIy >= s.H) break;
    } while (++iter < max_iters && err > eps2);
    if (fabsf(cIx - cTx) > kSubWin || fabsf(cIy - cTy) > kSubWin) {
        cIx = cTx;
        cIy = cTy;
    }
    if (lane == 0) {
        pt[0] = cIx;
        pt[1] = cIy;
        if (keep) {   // ORB::compute -> runByImageBorder(image.size(), edgeThreshold): Rect::contains(cvRound(pt))
            const int px = (int)rintf(cIx), py = (int)rintf(cIy);
            keep[k] = s.W > 2 * edge && s.H > 2 * edge && edge <= px && px < s.W - edge && edge <= py &&
                      py < s.H - edge;
        }
    }
}

/* ---------------- computeOrbDescriptors (WTA_K 2) on the blurred pyramid ----------------------------
 * One wave per keypoint, 4 ballots of 64 pair tests = 32 bytes.  Samples outside the level ROI read the
 * unblurred REFLECT_101 frame the reference's pyramid buffer holds around each (blurred) ROI. */
__global__ __launch_bounds__(256) void k_bird_desc(const BirdGeom* __restrict__ g, const uint8_t* __restrict__ pyr,
                                                   const uint8_t* __restrict__ blur, const int* __restrict__ pattern,
                                                   const orb_keypoint* __restrict__ kps, const int* __restrict__ keep,
                                                   int n, uint8_t* __restrict__ desc, const int* __restrict__ kframe,
                                                   unsigned fpitch) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= n) return;
    if (kframe) {   // batch: the pyramid and blurred pyramid of the keypoint's frame
        const size_t fo = (size_t)kframe[k] * fpitch;
        pyr += fo;
        blur += fo;
    }
    const orb_keypoint kp = kps[k];
    unsigned long long* out = reinterpret_cast<unsigned long long*>(desc + (long long)k * 32);
    if (keep && !keep[k]) {
        if (lane < 4) out[lane] = 0;
        return;
    }
    const BirdLevel L = g->L[kp.octave];
    const float scale = 1.f / L.scale;
    const int cy = (int)rintf(kp.y * scale), cx = (int)rintf(kp.x * scale);
    const float angle = kp.angle * kFactorPI;
    float a, b;
    glibc_sincosf(angle, &b, &a);   // cv::ORB's (float)cos / (float)sin of a float: glibc cosf / sinf
#pragma unroll
    for (int rnd = 0; rnd < 4; rnd++) {
        const int p = rnd * 64 + lane;   // pair p: points 2p, 2p+1 -> byte p/8, bit p%8
        int val[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int px = pattern[4 * p + 2 * q], py = pattern[4 * p + 2 * q + 1];
            const float x = px * a - py * b, y = px * b + py * a;
            const int sx = cx + (int)rintf(x), sy = cy + (int)rintf(y);
            if ((unsigned)sx < (unsigned)L.w && (unsigned)sy < (unsigned)L.h)
                val[q] = blur[L.off + (long long)sy * L.pitch + sx];
            else
                val[q] = pyr[L.off + (long long)reflect101_d(sy, L.h) * L.pitch + reflect101_d(sx, L.w)];
        }
        const unsigned long long m = __ballot(val[0] < val[1]);
        if (lane == 0) out[rnd] = m;
    }
}

#include "pattern31_data.inc"
const int kPattern31[1024] = {ORBGPU_PATTERN31_VALUES};

inline int cv_round(float v) { return (int)std::nearbyint(v); }
inline int cv_round(double v) { return (int)std::nearbyint(v); }

struct HostKP {   // cv::KeyPoint + the candidate it came from (payload only: the comparisons read response)
    float x, y, size, angle, response;
    int octave, class_id;
    int cand;
};

struct SelKey {   // (KeyPoint::response, candidate index)
    float response;
    int cand;
};

// KeyPointsFilter::retainBest (keypoint.cpp): nth_element + partition of the boundary ties
void retain_best(std::vector<SelKey>& kps, int n_points) {
    if (n_points >= 0 && kps.size() > (size_t)n_points) {
        if (n_points == 0) {
            kps.clear();
            return;
        }
        std::nth_element(kps.begin(), kps.begin() + n_points, kps.end(),
                         [](const SelKey& a, const SelKey& b) { return a.response > b.response; });
        const float amb = kps[n_points - 1].response;
        auto e = std::partition(kps.begin() + n_points, kps.end(),
                                [amb](const SelKey& k) { return k.response >= amb; });
        kps.resize(e - kps.begin());
    }
}

// what Bird::fetch_candidates hands the selection, per frame
struct BirdCands {
    std::vector<const BirdCand*> cands;       // the frame's candidates in level order (NULL: it has none)
    std::vector<int> lvl;                     // kBirdMaxLevels level counts per frame
    std::vector<size_t> total;                // their sum per frame
    std::vector<std::vector<BirdCand>> big;   // frames put together from the prefix and the second download
};

struct BatchFrame {   // keypoints [off, off + ns) of the device buffers are this frame's selection
    int frame, off, ns;
};

}  // namespace

struct Bird {
    int device = 0;
    hipStream_t stream = nullptr;
    int nfeatures = 2000, nlevels = 8, edge = 31, fastTh = 20, variant = 0;
    double scaleFactor = 1.2f;
    float wmask[kSubW * kSubW]{};

    bool have_geom = false;
    BirdGeom g{};
    long long pyr_bytes = 0;
    std::vector<int2> frows, crows, brows;   // FAST score rows, candidate rows, blur rows
    std::vector<int> lvl_row0;               // candidate-row range per level (nlevels + 1)
    std::vector<int> brow0;                  // blur-row range per level
    std::vector<int> rcoef_off;
    int max_w = 0;

    // device
    DevBuf<BirdGeom> d_geom;
    DevBuf<int2> d_rows;            // frows | crows | brows
    DevBuf<int> d_lvlrow0;
    DevBuf<ResizeCoef> d_rcoef;
    DevBuf<int> d_pattern;
    DevBuf<float> d_wmask;
    DevBuf<uint8_t> d_pyr, d_mpyr, d_score, d_blur;
    DevBuf<int> d_rowcnt, d_rowoff, d_lvlcnt;
    DevBuf<BirdCand> d_cand;        // (cap() >= cand_slot * nb_cap)
    size_t cand_slot = 0;           // candidates per frame of this geometry (the NMS bound)
    size_t cand_guess = 16384;      // candidates downloaded with the counts (next frame: this one's + 1/8)
    DevBuf<orb_keypoint> d_kps;
    DevBuf<int> d_keep;
    DevBuf<int> d_kframe;           // batch: frame of each keypoint
    DevBuf<uint8_t> d_desc;
    size_t kp_cap = 0;              // keypoints the four buffers above hold
    DevBuf<float> d_pts;

    // the pyramid, score, blur and row-count buffers hold nb_cap frames fpitch() bytes (or nr + 1 counts) apart,
    // the mask pyramid mnb_cap frames; the single calls are the one-frame case and use frame 0
    int nb_cap = 0, mnb_cap = 0;
    int batch_group = 4;            // frames whose keypoints go up in one upload + angle / subpix / desc launch
                                    // (measured, DESIGN 5.2: 2 .. 8 are within 5 % of each other, 1 and 64 lose more)
    // pinned staging: h_pin the level counts and candidate prefixes; h_up the keypoint uploads in device layout
    // (kp_cap keypoints, then kp_cap frame indices); h_res the second candidate download, then the results
    PinBuf<uint8_t> h_pin, h_up, h_res;
    orb_keypoint* up_kps() const { return (orb_keypoint*)h_up.get(); }
    int* up_frames() const { return (int*)(up_kps() + kp_cap); }
    unsigned fpitch() const { return (unsigned)pyr_bytes; }

    // host scratch of a call, members for their capacity (a warm call allocates nothing here): the candidates
    // fetch_candidates hands the selection, one frame's selection, the frames whose keypoints are in flight
    BirdCands cs;
    std::vector<HostKP> sel;
    std::vector<BatchFrame> done;

    // debug view of the last single detect / extract: candidates per level (empty after a batch call)
    std::vector<BirdCand> last_cands;
    std::vector<int> last_lvlcnt;

    ~Bird();
    void free_geom();
    int ensure_geometry(int W, int H, int nl, int nb = 1);
    int ensure_mask_frames(int n);
    int ensure_kp(size_t n);
    int reserve_kp(size_t n);
    int ensure_pinned(PinBuf<uint8_t>& p, size_t bytes);
    int upload(const uint8_t* img, size_t stride, const uint8_t* mask, size_t mstride, bool footprint, bool device_src,
               int frame = 0, int mask_frame = 0);
    int build_pyramid(int nl, bool with_mask, int nframes = 1, int nmasks = 1);
    int launch_candidates(bool with_mask, int nframes, bool per_frame_mask);
    void select(const BirdCand* cands, const int* lvlcnt, std::vector<HostKP>& sel) const;
    int fetch_candidates(int nframes, int nmasks, int blur_levels, bool debug_view);
    int upload_kps(int first, int n, bool frame_table);
    int launch_angle(int first, int n, const int* kframe);
    int launch_subpix(int first, int n, const int* kframe);
    int launch_blur(int nl, int nframes = 1);
    int launch_desc(int first, int n, bool keep, const int* kframe);
};

void Bird::free_geom() {
    d_geom.reset(), d_rows.reset(), d_lvlrow0.reset(), d_rcoef.reset();
    d_pyr.reset(), d_mpyr.reset(), d_score.reset(), d_blur.reset();
    d_rowcnt.reset(), d_rowoff.reset(), d_lvlcnt.reset();
    have_geom = false;
    nb_cap = mnb_cap = 0;
}

Bird::~Bird() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (stream) (void)hipStreamDestroy(stream);
}   // (the buffers free themselves: the device is current, the stream was idle)

// orb.cpp detectAndCompute: level sizes cvRound(cols / getScale(level)); nfeaturesPerLevel.  nb: frames
// the buffers must hold; a geometry keeps the largest batch it has seen.
int Bird::ensure_geometry(int W, int H, int nl, int nb) {
    const bool same = have_geom && g.W == W && g.H == H && g.nlevels == nl;
    if (same && nb <= nb_cap) return ORB_OK;
    if (same) nb = std::max(nb, nb_cap);
    hipError_t e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return set_error("sync", e), ORB_ERR_HIP;
    free_geom();
    BirdGeom G{};
    G.nlevels = nl;
    G.W = W;
    G.H = H;
    G.edge = edge;
    G.fastTh = std::min(std::max(fastTh, 0), 255);
    G.variant = variant;
    const float sc = 1.f / ((1 << 2) * 7 * 255.f);
    G.harris_scale4 = sc * sc * sc * sc;
    {   // getGaussianKernel(7, 2, CV_32F) -> 8-bit fixed point
        float cf[7];
        double s = 0;
        for (int i = 0; i < 7; i++) {
            const double x = i - 3.0;
            cf[i] = (float)std::exp(-0.5 / (2.0 * 2.0) * x * x);
            s += cf[i];
        }
        s = 1. / s;
        for (int i = 0; i < 7; i++) G.gk[i] = cv_round((float)(cf[i] * s) * 256.f);
    }
    {   // u_max (halfPatchSize 15)
        const int hp = 15;
        int umax[17];
        int v, v0, vmax = (int)std::floor(hp * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(hp * std::sqrt(2.f) / 2);
        for (v = 0; v <= vmax; ++v) umax[v] = cv_round(std::sqrt((double)hp * hp - v * v));
        for (v = hp, v0 = 0; v >= vmin; --v) {
            while (umax[v0] == umax[v0 + 1]) ++v0;
            umax[v] = v0;
            ++v0;
        }
        for (int i = 0; i < 16; i++) G.umax[i] = umax[i];
    }
    {   // nfeaturesPerLevel
        const float factor = (float)(1.0 / scaleFactor);
        float nd = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
        int sum = 0;
        for (int l = 0; l < nl - 1; l++) {
            G.L[l].nfeat = cv_round(nd);
            sum += G.L[l].nfeat;
            nd *= factor;
        }
        G.L[nl - 1].nfeat = std::max(nfeatures - sum, 0);
    }
    long long off = 0;
    frows.clear();
    crows.clear();
    brows.clear();
    lvl_row0.assign(nl + 1, 0);
    brow0.assign(nl + 1, 0);
    std::vector<ResizeCoef> coefs;
    rcoef_off.assign(nl, 0);
    max_w = 0;
    for (int l = 0; l < nl; l++) {
        BirdLevel& L = G.L[l];
        L.scale = (float)std::pow(scaleFactor, (double)l);
        L.w = cv_round((float)W / L.scale);
        L.h = cv_round((float)H / L.scale);
        if (L.w < 1 || L.h < 1) return set_error("birdview image too small for the pyramid", hipSuccess), ORB_ERR_GEOMETRY;
        L.pitch = (L.w + 63) & ~63;
        L.off = off;
        off += (long long)L.pitch * L.h + 256;
        max_w = std::max(max_w, L.w);
        lvl_row0[l] = (int)crows.size();
        brow0[l] = (int)brows.size();
        // runByImageBorder clears a level with h <= 2e or w <= 2e; FAST needs the 3-pixel ring
        if (L.w > 2 * edge && L.h > 2 * edge && edge >= 4) {
            for (int y = edge - 1; y <= L.h - edge; y++) frows.push_back(make_int2(l, y));
            for (int y = edge; y < L.h - edge; y++) crows.push_back(make_int2(l, y));
        }
        for (int y = 0; y < L.h; y++) brows.push_back(make_int2(l, y));
        if (l > 0) {
            rcoef_off[l] = (int)coefs.size();
            resize_coefs(G.L[l - 1].w, L.w, coefs, false);
            resize_coefs(G.L[l - 1].h, L.h, coefs, true);
        }
    }
    if (edge < 4) return set_error("edgeThreshold < 4 is not supported", hipSuccess), ORB_ERR_ARG;
    lvl_row0[nl] = (int)crows.size();
    brow0[nl] = (int)brows.size();
    // frame f of a batch is addressed as base + f * pyr_bytes with 32-bit level offsets
    if (off >= (1ll << 31)) return set_error("birdview image too large", hipSuccess), ORB_ERR_GEOMETRY;
    pyr_bytes = off;
    g = G;
    std::vector<int2> rows(frows);
    rows.insert(rows.end(), crows.begin(), crows.end());
    rows.insert(rows.end(), brows.begin(), brows.end());
    const size_t nr = crows.size();
    size_t ccap = 0;   // NMS survivors never touch: <= ceil(w/2) * ceil(h/2) per level
    for (int l = 0; l < nl; l++) ccap += (size_t)((G.L[l].w + 1) / 2) * ((G.L[l].h + 1) / 2);
    if ((e = d_geom.ensure(1)) != hipSuccess || (e = d_rows.ensure(std::max<size_t>(rows.size(), 1))) != hipSuccess ||
        (e = d_lvlrow0.ensure(nl + 1)) != hipSuccess ||
        (e = d_rcoef.ensure(std::max<size_t>(coefs.size(), 1))) != hipSuccess ||
        (e = d_pyr.ensure((size_t)pyr_bytes * nb)) != hipSuccess || (e = d_mpyr.ensure(pyr_bytes)) != hipSuccess ||
        (e = d_score.ensure((size_t)pyr_bytes * nb)) != hipSuccess ||
        (e = d_blur.ensure((size_t)pyr_bytes * nb)) != hipSuccess ||
        (e = d_rowcnt.ensure((nr + 1) * nb)) != hipSuccess || (e = d_rowoff.ensure((nr + 1) * nb)) != hipSuccess ||
        (e = d_lvlcnt.ensure((size_t)kBirdMaxLevels * nb)) != hipSuccess)
        return free_geom(), set_error("birdview buffers", e), ORB_ERR_NOMEM;
    cand_slot = ccap;
    if ((e = d_cand.ensure(ccap * nb)) != hipSuccess)
        return free_geom(), set_error("birdview candidates", e), ORB_ERR_NOMEM;
    if ((e = hipMemcpyAsync(d_geom.get(), &g, sizeof(BirdGeom), hipMemcpyHostToDevice, stream)) != hipSuccess ||
        (!rows.empty() &&
         (e = hipMemcpyAsync(d_rows.get(), rows.data(), rows.size() * sizeof(int2), hipMemcpyHostToDevice, stream)) !=
             hipSuccess) ||
        (e = hipMemcpyAsync(d_lvlrow0.get(), lvl_row0.data(), (nl + 1) * sizeof(int), hipMemcpyHostToDevice, stream)) !=
            hipSuccess ||
        (!coefs.empty() && (e = hipMemcpyAsync(d_rcoef.get(), coefs.data(), coefs.size() * sizeof(ResizeCoef),
                                               hipMemcpyHostToDevice, stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(stream)) != hipSuccess)
        return free_geom(), set_error("birdview geometry upload", e), ORB_ERR_HIP;
    have_geom = true;
    nb_cap = nb;
    mnb_cap = 1;
    return ORB_OK;
}

// per-frame masks: one mask pyramid per frame (a shared mask needs the one ensure_geometry allocates)
int Bird::ensure_mask_frames(int n) {
    if (n <= mnb_cap) return ORB_OK;
    hipError_t e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return set_error("sync", e), ORB_ERR_HIP;
    mnb_cap = 0;
    if ((e = d_mpyr.ensure((size_t)pyr_bytes * n)) != hipSuccess) {
        // the geometry cannot stay without its mask pyramid
        return free_geom(), set_error("birdview mask pyramids", e), ORB_ERR_NOMEM;
    }
    mnb_cap = n;
    return ORB_OK;
}

// nothing may be in flight on the keypoint buffers when they grow
int Bird::ensure_kp(size_t n) {
    if (n <= kp_cap && d_kps) return ORB_OK;
    const size_t cap = std::max<size_t>(n, 4096);
    d_kps.reset(), d_keep.reset(), d_kframe.reset(), d_desc.reset();   // (all four go before any comes back)
    kp_cap = 0;
    hipError_t e;
    if ((e = d_kps.ensure(cap)) != hipSuccess || (e = d_keep.ensure(cap)) != hipSuccess ||
        (e = d_kframe.ensure(cap)) != hipSuccess || (e = d_desc.ensure(cap * 32)) != hipSuccess)
        return set_error("birdview keypoint buffers", e), ORB_ERR_NOMEM;
    kp_cap = cap;
    return ORB_OK;
}

int Bird::ensure_pinned(PinBuf<uint8_t>& p, size_t bytes) {
    const hipError_t e = p.ensure(bytes, 1 << 20);
    if (e != hipSuccess) return set_error("pinned staging", e), ORB_ERR_NOMEM;
    return ORB_OK;
}

// keypoint buffers for n keypoints and the pinned staging their upload comes from
int Bird::reserve_kp(size_t n) {
    const int r = ensure_kp(n);
    return r != ORB_OK ? r : ensure_pinned(h_up, kp_cap * (sizeof(orb_keypoint) + sizeof(int)));
}

// Frame.cc:320-327 footprint rectangle (doubles truncated into cv::Rect, filled, clipped)
static void footprint_rect(int W, int H, int& x0, int& y0, int& x1, int& y1) {
    const double p2m = 0.03984 * 1.7, len = 4.63, wid = 1.901, boundary = 15.0;
    const double x = W / 2 - (wid / 2 / p2m) - boundary, y = H / 2 - (len / 2 / p2m) - boundary;
    const double width = wid / p2m + 2 * boundary, height = len / p2m + 2 * boundary;
    const int rx = (int)x, ry = (int)y, rw = (int)width, rh = (int)height;
    if (rw <= 0 || rh <= 0) {
        x0 = y0 = x1 = y1 = 0;
        return;
    }
    x0 = std::max(rx, 0);
    y0 = std::max(ry, 0);
    x1 = std::min(rx + rw, W);
    y1 = std::min(ry + rh, H);
}

// img (may be NULL: mask only) into level 0 of pyramid `frame`, mask into level 0 of mask pyramid `mask_frame`
int Bird::upload(const uint8_t* img, size_t stride, const uint8_t* mask, size_t mstride, bool footprint,
                 bool device_src, int frame, int mask_frame) {
    const hipMemcpyKind kind = device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const BirdLevel& L0 = g.L[0];
    hipError_t e;
    if (img && (e = hipMemcpy2DAsync(d_pyr.get() + (size_t)frame * pyr_bytes + L0.off, L0.pitch, img, stride, L0.w, L0.h, kind,
                                     stream)) != hipSuccess)
        return set_error("birdview image upload", e), ORB_ERR_HIP;
    if (mask) {
        uint8_t* m0 = d_mpyr.get() + (size_t)mask_frame * pyr_bytes + L0.off;
        if ((e = hipMemcpy2DAsync(m0, L0.pitch, mask, mstride, L0.w, L0.h, kind, stream)) != hipSuccess)
            return set_error("birdview mask upload", e), ORB_ERR_HIP;
        if (footprint) {
            int x0, y0, x1, y1;
            footprint_rect(L0.w, L0.h, x0, y0, x1, y1);
            if (x1 > x0 && y1 > y0 &&
                (e = hipMemset2DAsync(m0 + (long long)y0 * L0.pitch + x0, L0.pitch, 0, x1 - x0, y1 - y0,
                                      stream)) != hipSuccess)
                return set_error("footprint", e), ORB_ERR_HIP;
        }
    }
    return ORB_OK;
}

// one launch per level: nframes image pyramids and, with a mask, nmasks (1: shared, or nframes) mask pyramids
int Bird::build_pyramid(int nl, bool with_mask, int nframes, int nmasks) {
    for (int l = 1; l < nl; l++) {
        dim3 grid((g.L[l].w + 255) / 256, g.L[l].h, nframes + (with_mask ? nmasks : 0));
        hipLaunchKernelGGL(k_bird_resize, grid, dim3(256), 0, stream, d_geom.get(), l, d_rcoef.get() + rcoef_off[l], d_pyr.get(), d_mpyr.get(),
                           nframes, fpitch());
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error("k_bird_resize", e), ORB_ERR_HIP;
    return ORB_OK;
}

// FAST score map, count / scan / emit for nframes frames (crows is not empty)
int Bird::launch_candidates(bool with_mask, int nframes, bool per_frame_mask) {
    const int nl = g.nlevels;
    const int nf = (int)frows.size(), nc = (int)crows.size();
    const int2* d_frows = d_rows.get();
    const int2* d_crows = d_rows.get() + nf;
    const int fx = (max_w - 2 * edge + 2 + 255) / 256;
    const unsigned fp = fpitch(), mfp = per_frame_mask ? fp : 0u, slot = (unsigned)cand_slot;
    hipLaunchKernelGGL(k_bird_fast, dim3(std::max(fx, 1), nf, nframes), dim3(256), 0, stream, d_geom.get(), d_frows, d_pyr.get(),
                       d_score.get(), fp);
    const uint8_t* mp = with_mask ? d_mpyr.get() : nullptr;
    hipLaunchKernelGGL(k_bird_cands<0>, dim3((nc + 3) / 4, nframes), dim3(256), 0, stream, d_geom.get(), d_crows, nc, d_pyr.get(),
                       mp, d_score.get(), d_rowcnt.get(), (const int*)nullptr, (BirdCand*)nullptr, fp, mfp, slot);
    hipLaunchKernelGGL(k_bird_scan, dim3(nframes), dim3(1024), 0, stream, d_rowcnt.get(), nc, d_lvlrow0.get(), nl, d_rowoff.get(),
                       d_lvlcnt.get());
    hipLaunchKernelGGL(k_bird_cands<1>, dim3((nc + 3) / 4, nframes), dim3(256), 0, stream, d_geom.get(), d_crows, nc, d_pyr.get(),
                       mp, d_score.get(), (int*)nullptr, d_rowoff.get(), d_cand.get(), fp, mfp, slot);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error("birdview FAST", e), ORB_ERR_HIP;
    return ORB_OK;
}

// computeKeyPoints up to the selection, for nframes frames whose pyramids (and nmasks = 0, 1 or nframes mask
// pyramids) are built: the candidate launches, the blurred pyramid of blur_levels levels behind them (it only
// needs the pyramid, so it runs while the host selects), then one download of every frame's level counts and
// speculative candidate prefix (sized from the previous call) and one synchronise; the frames that have more get
// a second download together.  debug_view (one frame): the frame's candidates are put together in last_cands /
// last_lvlcnt, which orb_bird_debug_candidates reads; otherwise those are left empty.  The result is in cs.
int Bird::fetch_candidates(int nframes, int nmasks, int blur_levels, bool debug_view) {
    const int nl = g.nlevels, B = nframes;
    BirdCands& out = cs;
    std::vector<size_t>& total = out.total;
    int r;
    hipError_t e;
    out.cands.assign(B, nullptr);
    out.lvl.assign((size_t)B * kBirdMaxLevels, 0);
    total.assign(B, 0);
    out.big.clear();
    last_lvlcnt.assign(debug_view ? nl : 0, 0);
    last_cands.clear();
    if (crows.empty()) return blur_levels > 0 ? launch_blur(blur_levels, B) : ORB_OK;
    if ((r = launch_candidates(nmasks > 0, B, nmasks > 1)) != ORB_OK) return r;
    if (blur_levels > 0 && (r = launch_blur(blur_levels, B)) != ORB_OK) return r;
    const size_t slot = cand_slot, guess = std::min(cand_guess, slot);
    const size_t cnt_bytes = (size_t)B * kBirdMaxLevels * sizeof(int), hdr = (cnt_bytes + 63) & ~(size_t)63;
    if ((r = ensure_pinned(h_pin, hdr + (size_t)B * guess * sizeof(BirdCand))) != ORB_OK) return r;
    const int* cnt = (const int*)h_pin.get();
    BirdCand* pre = (BirdCand*)(h_pin.get() + hdr);
    if ((e = hipMemcpyAsync(h_pin.get(), d_lvlcnt.get(), cnt_bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess)
        return set_error("birdview count download", e), ORB_ERR_HIP;
    for (int f = 0; f < B && guess; f++)
        if ((e = hipMemcpyAsync(pre + f * guess, d_cand.get() + f * slot, guess * sizeof(BirdCand), hipMemcpyDeviceToHost,
                                stream)) != hipSuccess)
            return set_error("birdview candidate download", e), ORB_ERR_HIP;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return set_error("birdview candidate download", e), ORB_ERR_HIP;
    size_t rest_total = 0, max_total = 0;
    for (int f = 0; f < B; f++) {
        for (int l = 0; l < nl; l++) {
            const int i = f * kBirdMaxLevels + l;
            out.lvl[i] = cnt[i];
            total[f] += cnt[i];
        }
        if (total[f] > slot) return set_error("birdview candidate overflow", hipSuccess), ORB_ERR_INTERNAL;
        out.cands[f] = pre + f * guess;
        if (total[f] > guess) rest_total += total[f] - guess;
        max_total = std::max(max_total, total[f]);
    }
    if (rest_total) {
        if ((r = ensure_pinned(h_res, rest_total * sizeof(BirdCand))) != ORB_OK) return r;
        BirdCand* hr = (BirdCand*)h_res.get();
        for (int f = 0; f < B; f++)
            if (total[f] > guess) {
                const size_t rest = total[f] - guess;
                if ((e = hipMemcpyAsync(hr, d_cand.get() + f * slot + guess, rest * sizeof(BirdCand), hipMemcpyDeviceToHost,
                                        stream)) != hipSuccess)
                    return set_error("birdview candidates download", e), ORB_ERR_HIP;
                hr += rest;
            }
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return set_error("birdview candidates download", e), ORB_ERR_HIP;
        if (!debug_view) out.big.resize(B);
    }
    // a frame above the prefix is put together on the host; so is the frame of the debug view (hr walks the second
    // download and is read only where a frame has a rest, that is, only when rest_total > 0 has allocated h_res)
    const BirdCand* hr = (const BirdCand*)h_res.get();
    for (int f = 0; f < B; f++)
        if (total[f] > guess || debug_view) {
            std::vector<BirdCand>& all = debug_view ? last_cands : out.big[f];
            const size_t head = std::min(total[f], guess), rest = total[f] - head;
            all.resize(total[f]);
            if (head) std::memcpy(all.data(), pre + f * guess, head * sizeof(BirdCand));
            if (rest) std::memcpy(all.data() + head, hr, rest * sizeof(BirdCand));
            hr += rest;
            out.cands[f] = all.data();
        }
    if (debug_view) last_lvlcnt.assign(out.lvl.begin(), out.lvl.begin() + nl);
    cand_guess = max_total + max_total / 8 + 256;
    return ORB_OK;
}

// KeyPointsFilter::retainBest(2 N) on the FAST response, per level; then Harris, retainBest(N).
// nth_element / partition see only the responses, so they run on 8-byte (response, candidate)
// keys: the resulting arrangement is the one a vector<cv::KeyPoint> gets.
void Bird::select(const BirdCand* cands, const int* lvlcnt, std::vector<HostKP>& sel) const {
    const int nl = g.nlevels;
    std::vector<std::vector<SelKey>> lv(nl);
    size_t off = 0;
    for (int l = 0; l < nl; l++) {
        auto& k = lv[l];
        k.resize(lvlcnt[l]);
        for (int i = 0; i < lvlcnt[l]; i++) k[i] = {(float)cands[off + i].score, (int)(off + i)};
        off += lvlcnt[l];
        retain_best(k, 2 * g.L[l].nfeat);
    }
    size_t any = 0;
    for (int l = 0; l < nl; l++) any += lv[l].size();
    if (!any) return;
    for (int l = 0; l < nl; l++) {
        for (auto& kp : lv[l]) kp.response = cands[kp.cand].harris;
        retain_best(lv[l], g.L[l].nfeat);
        const float size = 31 * g.L[l].scale;
        for (const auto& kp : lv[l]) {
            const BirdCand& c = cands[kp.cand];
            sel.push_back({(float)(c.xy & 0xFFFF), (float)(c.xy >> 16), size, -1.f, kp.response, l, -1, kp.cand});
        }
    }
}

// keypoints [first, first + n) of the pinned staging to the device, with their frame indices for a frame table
int Bird::upload_kps(int first, int n, bool frame_table) {
    hipError_t e;
    if (n && ((e = hipMemcpyAsync(d_kps.get() + first, up_kps() + first, (size_t)n * sizeof(orb_keypoint),
                                  hipMemcpyHostToDevice, stream)) != hipSuccess ||
              (frame_table && (e = hipMemcpyAsync(d_kframe.get() + first, up_frames() + first, (size_t)n * sizeof(int),
                                                  hipMemcpyHostToDevice, stream)) != hipSuccess)))
        return set_error("birdview keypoint upload", e), ORB_ERR_HIP;
    return ORB_OK;
}

// The per-keypoint launches work on keypoints [first, first + n) of the device buffers.  kframe: the frame of each
// of them (a pointer into d_kframe), or NULL when the call has one frame: then the kernels read frame 0 and no
// frame pitch.
int Bird::launch_angle(int first, int n, const int* kframe) {
    if (n)
        hipLaunchKernelGGL(k_bird_angle, dim3((n + 3) / 4), dim3(256), 0, stream, d_geom.get(), d_pyr.get(), d_kps.get() + first, n,
                           kframe, kframe ? fpitch() : 0u);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ORB_OK : (set_error("k_bird_angle", e), ORB_ERR_HIP);
}

// cornerSubPix on the level-0 image of the keypoint's frame, with the border (keep) flag
int Bird::launch_subpix(int first, int n, const int* kframe) {
    SubpixSrc s{d_pyr.get() + g.L[0].off, g.L[0].pitch, g.L[0].w, g.L[0].h};
    if (n)
        hipLaunchKernelGGL(k_bird_subpix, dim3((n + 3) / 4), dim3(256), 0, stream, s, d_wmask.get(),
                           reinterpret_cast<float*>(d_kps.get() + first), 7, n, 40, 0.001 * 0.001, edge, d_keep.get() + first,
                           kframe, kframe ? fpitch() : 0u);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ORB_OK : (set_error("k_bird_subpix", e), ORB_ERR_HIP);
}

int Bird::launch_blur(int nl, int nframes) {
    const int2* d_brows = d_rows.get() + frows.size() + crows.size();
    const int nb = brow0[nl];
    if (nb)
        hipLaunchKernelGGL(k_bird_blur, dim3((max_w + 255) / 256, nb, nframes), dim3(256), 0, stream, d_geom.get(), d_brows,
                           d_pyr.get(), d_blur.get(), fpitch());
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ORB_OK : (set_error("k_bird_blur", e), ORB_ERR_HIP);
}

// descriptors on the blurred pyramid; keep: zero those of the keypoints launch_subpix flagged as culled
int Bird::launch_desc(int first, int n, bool keep, const int* kframe) {
    if (n)
        hipLaunchKernelGGL(k_bird_desc, dim3((n + 3) / 4), dim3(256), 0, stream, d_geom.get(), d_pyr.get(), d_blur.get(), d_pattern.get(),
                           d_kps.get() + first, keep ? d_keep.get() + first : nullptr, n, d_desc.get() + (size_t)first * 32, kframe,
                           kframe ? fpitch() : 0u);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ORB_OK : (set_error("k_bird_desc", e), ORB_ERR_HIP);
}

}  // namespace orbgpu

using namespace orbgpu;

struct orb_bird : Bird {};

static int bird_enter(orb_bird* b) {
    if (!b) return set_error("NULL orb_bird", hipSuccess), ORB_ERR_ARG;
    hipError_t e = hipSetDevice(b->device);
    if (e != hipSuccess) return set_error("hipSetDevice", e), ORB_ERR_HIP;
    return ORB_OK;
}

extern "C" orb_bird* orb_bird_create(const orb_bird_params* p, int* status) {
    auto fail = [&](int st) -> orb_bird* {
        if (status) *status = st;
        return nullptr;
    };
    if (!p || p->nfeatures < 0 || p->nlevels < 1 || p->nlevels > ORBGPU_MAX_LEVELS || !(p->scaleFactor > 1.0f) ||
        p->edgeThreshold < 4 || p->fastThreshold < 0 ||
        (p->variant & ~(ORB_VARIANT_RESIZE_GENERIC | ORB_VARIANT_BLUR_HALFUP))) {
        set_error("invalid orb_bird_params", hipSuccess);
        return fail(ORB_ERR_ARG);
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || p->device < 0 || p->device >= ndev) {
        set_error("no HIP device (liborbgpu has no CPU fallback)", e);
        return fail(ORB_ERR_HIP);
    }
    if ((e = hipSetDevice(p->device)) != hipSuccess) return set_error("hipSetDevice", e), fail(ORB_ERR_HIP);
    orb_bird* b = new (std::nothrow) orb_bird();
    if (!b) return fail(ORB_ERR_NOMEM);
    b->device = p->device;
    b->nfeatures = p->nfeatures;
    b->scaleFactor = p->scaleFactor;
    b->nlevels = p->nlevels;
    b->edge = p->edgeThreshold;
    b->fastTh = p->fastThreshold;
    b->variant = p->variant;
    // cornerSubPix weight mask: exp(-y^2) * exp(-x^2) in float (glibc expf, as the reference's host)
    for (int i = 0; i < kSubW; i++) {
        const float y = (float)(i - kSubWin) / kSubWin;
        const float vy = std::exp(-y * y);
        for (int j = 0; j < kSubW; j++) {
            const float x = (float)(j - kSubWin) / kSubWin;
            b->wmask[i * kSubW + j] = (float)(vy * std::exp(-x * x));
        }
    }
    if ((e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = b->d_pattern.ensure(sizeof(kPattern31) / sizeof(int))) != hipSuccess ||
        (e = b->d_wmask.ensure(kSubW * kSubW)) != hipSuccess ||
        (e = hipMemcpyAsync(b->d_pattern.get(), kPattern31, sizeof(kPattern31), hipMemcpyHostToDevice, b->stream)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(b->d_wmask.get(), b->wmask, sizeof(b->wmask), hipMemcpyHostToDevice, b->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(b->stream)) != hipSuccess) {
        delete b;
        set_error("orb_bird_create", e);
        return fail(ORB_ERR_HIP);
    }
    if (status) *status = ORB_OK;
    return b;
}

extern "C" void orb_bird_destroy(orb_bird* b) {
    if (b) delete b;
}

extern "C" int orb_bird_footprint_mask(uint8_t* mask, int w, int h, size_t stride) {
    if (!mask || w < 0 || h < 0 || stride < (size_t)w) return set_error("orb_bird_footprint_mask: bad arguments", hipSuccess), ORB_ERR_ARG;
    int x0, y0, x1, y1;
    footprint_rect(w, h, x0, y0, x1, y1);
    for (int y = y0; y < y1; y++) std::memset(mask + (size_t)y * stride + x0, 0, x1 - x0);
    return ORB_OK;
}

static void to_kp(const HostKP& h, orb_keypoint& k) {
    k.x = h.x;
    k.y = h.y;
    k.size = h.size;
    k.angle = h.angle;
    k.response = h.response;
    k.octave = h.octave;
    k.class_id = h.class_id;
}

/* ---------------- the host body: nframes images of one size through the chain in one call --------------
 * Every stage before the selection is one launch over all frames; the selection runs frame by frame on
 * the host, and the keypoints of each group of batch_group frames go up and through angle / subpix / desc
 * while the host selects the next group.  One synchronise for the candidates, one at the end.  The single
 * calls are the case of one frame: no frame table is written or uploaded, the kernels get kframe == NULL. */
// download everything launched so far; compact each frame by its keep flags into the caller's slot
static int bird_batch_flush(orb_bird* b, std::vector<BatchFrame>& done, int used, orb_keypoint* kps, uint8_t* desc,
                            int cap, int* counts, bool& over) {
    int r;
    hipError_t e;
    const size_t kb = (size_t)used * sizeof(orb_keypoint), fb = (size_t)used * sizeof(int), db = (size_t)used * 32;
    if ((r = b->ensure_pinned(b->h_res, kb + fb + db + 64)) != ORB_OK) return r;
    uint8_t* hp = b->h_res.get();
    if (used && ((e = hipMemcpyAsync(hp, b->d_kps.get(), kb, hipMemcpyDeviceToHost, b->stream)) != hipSuccess ||
                 (e = hipMemcpyAsync(hp + kb, b->d_keep.get(), fb, hipMemcpyDeviceToHost, b->stream)) != hipSuccess ||
                 (e = hipMemcpyAsync(hp + kb + fb, b->d_desc.get(), db, hipMemcpyDeviceToHost, b->stream)) != hipSuccess))
        return set_error("birdview result download", e), ORB_ERR_HIP;
    if ((e = hipStreamSynchronize(b->stream)) != hipSuccess) return set_error("birdview sync", e), ORB_ERR_HIP;
    const orb_keypoint* rk = (const orb_keypoint*)hp;
    const int* keep = (const int*)(hp + kb);
    const uint8_t* rd = hp + kb + fb;
    for (const BatchFrame& q : done) {
        int m = 0;
        for (int i = q.off; i < q.off + q.ns; i++) m += keep[i] != 0;
        counts[q.frame] = m;
        if (m > cap) {   // this frame's slot stays untouched
            over = true;
            continue;
        }
        orb_keypoint* ok = kps + (size_t)q.frame * cap;
        uint8_t* od = desc + (size_t)q.frame * cap * 32;
        for (int i = q.off, j = 0; i < q.off + q.ns; i++)
            if (keep[i]) {
                ok[j] = rk[i];
                std::memcpy(od + (size_t)j * 32, rd + (size_t)i * 32, 32);
                j++;
            }
    }
    done.clear();
    return ORB_OK;
}

// Frame.cc:329-342 for B frames: level 0 of every frame, and of nmasks = 0, 1 or B footprint-zeroed masks, is in
// its slot, and bird_reserve has run.  fn names the entry point in the capacity error.  debug_view: see
// Bird::fetch_candidates.
static int bird_body(orb_bird* b, const char* fn, int B, int nmasks, bool debug_view, orb_keypoint* kps, uint8_t* desc,
                     int cap, int* counts) {
    int r;
    const int nl = b->g.nlevels;
    if ((r = b->build_pyramid(nl, nmasks > 0, B, std::max(nmasks, 1))) != ORB_OK) return r;
    // every level is blurred (compute() would blur max octave + 1 of them; the extra levels are never read)
    if ((r = b->fetch_candidates(B, nmasks, nl, debug_view)) != ORB_OK) return r;
    const BirdCands& c = b->cs;

    // selection frame by frame; each full group goes up and through its kernels behind the host
    std::vector<BatchFrame>& done = b->done;
    std::vector<HostKP>& sel = b->sel;
    done.clear();
    int used = 0, g0 = 0, gframes = 0;
    bool over = false;
    const bool frame_table = B > 1;
    auto launch_group = [&]() -> int {
        const int n = used - g0;
        const int* kf = frame_table ? b->d_kframe.get() + g0 : nullptr;
        int lr;
        if (n && ((lr = b->upload_kps(g0, n, frame_table)) != ORB_OK || (lr = b->launch_angle(g0, n, kf)) != ORB_OK ||
            (lr = b->launch_subpix(g0, n, kf)) != ORB_OK || (lr = b->launch_desc(g0, n, true, kf)) != ORB_OK))
            return lr;
        g0 = used;
        gframes = 0;
        return ORB_OK;
    };
    for (int f = 0; f < B; f++) {
        sel.clear();
        if (c.cands[f]) b->select(c.cands[f], &c.lvl[(size_t)f * kBirdMaxLevels], sel);
        const int ns = (int)sel.size();
        if ((size_t)used + ns > b->kp_cap) {
            // boundary ties kept more than nfeatures per frame: drain what is in flight, then grow if needed
            if ((r = launch_group()) != ORB_OK ||
                (r = bird_batch_flush(b, done, used, kps, desc, cap, counts, over)) != ORB_OK)
                return r;
            used = g0 = 0;
            if ((r = b->reserve_kp(ns)) != ORB_OK) return r;
        }
        for (int i = 0; i < ns; i++) to_kp(sel[i], b->up_kps()[used + i]);
        if (frame_table) std::fill_n(b->up_frames() + used, ns, f);
        done.push_back({f, used, ns});
        used += ns;
        if (++gframes >= b->batch_group && (r = launch_group()) != ORB_OK) return r;
    }
    if ((r = launch_group()) != ORB_OK) return r;
    if ((r = bird_batch_flush(b, done, used, kps, desc, cap, counts, over)) != ORB_OK) return r;
    if (over) return set_error((std::string(fn) + ": capacity").c_str(), hipSuccess), ORB_ERR_CAPACITY;
    return ORB_OK;
}

// argument rules of detect, extract and the batch forms, named fn in the messages (a single call is nframes 1 with
// its count as counts); *done: the call is complete (nothing to do)
static int bird_frames_enter(orb_bird* b, const char* fn, int nframes, const void* imgs, int w, int h, size_t stride,
                             size_t frame_pitch, bool with_mask, size_t mask_stride, size_t mask_frame_pitch,
                             const orb_keypoint* kps, const uint8_t* desc, bool need_desc, int cap, int* counts,
                             bool* done) {
    *done = true;
    if (!b) return set_error("NULL orb_bird", hipSuccess), ORB_ERR_ARG;
    if (nframes < 0 || nframes > ORB_BIRD_MAX_BATCH || !counts || cap < 0 || (cap && (!kps || (need_desc && !desc))))
        return arg_error(fn, "bad arguments");
    if (nframes == 0) return ORB_OK;
    if (!imgs || w <= 0 || h <= 0) {   // Feature2D::detect: empty image -> keypoints.clear()
        for (int f = 0; f < nframes; f++) counts[f] = 0;
        return ORB_OK;
    }
    if (stride < (size_t)w || frame_pitch < stride * (size_t)h ||
        (with_mask && (mask_stride < (size_t)w || (mask_frame_pitch && mask_frame_pitch < mask_stride * (size_t)h))))
        return arg_error(fn, "bad strides");
    int r;
    if ((r = bird_enter(b)) != ORB_OK) return r;
    *done = false;
    return ORB_OK;
}

// buffers for B frames of w x h with nmasks mask pyramids, keypoint buffers for the expected selection
static int bird_reserve(orb_bird* b, int B, int w, int h, int nmasks) {
    int r;
    if ((r = b->ensure_geometry(w, h, b->nlevels, B)) != ORB_OK) return r;
    if ((r = b->ensure_mask_frames(nmasks)) != ORB_OK) return r;
    return b->reserve_kp((size_t)B * ((size_t)b->nfeatures + 64));
}

extern "C" int orb_bird_detect(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, const uint8_t* mask,
                               size_t mask_stride, orb_keypoint* kps, int cap, int* n) {
    static const char* fn = "orb_bird_detect";
    int r;
    bool done;
    if ((r = bird_frames_enter(b, fn, 1, img, w, h, stride, stride * (size_t)(h > 0 ? h : 0), mask != nullptr, mask_stride,
                               0, kps, nullptr, false, cap, n, &done)) != ORB_OK ||
        done)
        return r;
    const int nmasks = mask ? 1 : 0;
    if ((r = b->ensure_geometry(w, h, b->nlevels)) != ORB_OK) return r;
    if ((r = b->upload(img, stride, mask, mask_stride, false, false)) != ORB_OK) return r;
    if ((r = b->build_pyramid(b->g.nlevels, nmasks > 0)) != ORB_OK) return r;
    if ((r = b->fetch_candidates(1, nmasks, 0, true)) != ORB_OK) return r;
    const BirdCands& c = b->cs;
    std::vector<HostKP>& sel = b->sel;
    sel.clear();
    if (c.cands[0]) b->select(c.cands[0], c.lvl.data(), sel);
    const int ns = (int)sel.size();
    *n = ns;
    if (ns > cap) return set_error("orb_bird_detect: capacity", hipSuccess), ORB_ERR_CAPACITY;
    if ((r = b->reserve_kp(std::max(ns, 1))) != ORB_OK) return r;
    for (int i = 0; i < ns; i++) to_kp(sel[i], b->up_kps()[i]);
    if ((r = b->upload_kps(0, ns, false)) != ORB_OK || (r = b->launch_angle(0, ns, nullptr)) != ORB_OK) return r;
    hipError_t e;
    if (ns && ((e = hipMemcpyAsync(kps, b->d_kps.get(), ns * sizeof(orb_keypoint), hipMemcpyDeviceToHost, b->stream)) !=
                   hipSuccess ||
               (e = hipStreamSynchronize(b->stream)) != hipSuccess))
        return set_error("birdview keypoint download", e), ORB_ERR_HIP;
    return ORB_OK;
}

// the fused single call: one frame of the body, level 0 by strided copies from the host or the device
static int bird_extract(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, const uint8_t* mask,
                        size_t mask_stride, orb_keypoint* kps, int cap, int* n, uint8_t* desc, bool device_src) {
    static const char* fn = "orb_bird_extract";
    int r;
    bool done;
    if ((r = bird_frames_enter(b, fn, 1, img, w, h, stride, stride * (size_t)(h > 0 ? h : 0), mask != nullptr, mask_stride,
                               0, kps, desc, true, cap, n, &done)) != ORB_OK ||
        done)
        return r;
    const int nmasks = mask ? 1 : 0;
    if ((r = bird_reserve(b, 1, w, h, nmasks)) != ORB_OK) return r;
    if ((r = b->upload(img, stride, mask, mask_stride, true, device_src)) != ORB_OK) return r;
    return bird_body(b, fn, 1, nmasks, true, kps, desc, cap, n);
}

extern "C" int orb_bird_extract(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, const uint8_t* mask,
                                size_t mask_stride, orb_keypoint* kps, int cap, int* n, uint8_t* desc) {
    return bird_extract(b, img, w, h, stride, mask, mask_stride, kps, cap, n, desc, false);
}

extern "C" int orb_bird_extract_device(orb_bird* b, const uint8_t* d_img, int w, int h, size_t stride,
                                       const uint8_t* d_mask, size_t mask_stride, orb_keypoint* kps, int cap, int* n,
                                       uint8_t* desc) {
    return bird_extract(b, d_img, w, h, stride, d_mask, mask_stride, kps, cap, n, desc, true);
}

extern "C" int orb_bird_extract_batch_device(orb_bird* b, int nframes, const uint8_t* d_imgs, int w, int h,
                                             size_t stride, size_t frame_pitch, const uint8_t* d_masks,
                                             size_t mask_stride, size_t mask_frame_pitch, orb_keypoint* kps,
                                             uint8_t* desc, int cap, int* counts) {
    static const char* fn = "orb_bird_extract_batch";
    int r;
    bool done;
    if ((r = bird_frames_enter(b, fn, nframes, d_imgs, w, h, stride, frame_pitch, d_masks != nullptr, mask_stride,
                               mask_frame_pitch, kps, desc, true, cap, counts, &done)) != ORB_OK ||
        done)
        return r;
    const int nmasks = !d_masks ? 0 : (mask_frame_pitch ? nframes : 1);
    if ((r = bird_reserve(b, nframes, w, h, nmasks)) != ORB_OK) return r;
    int x0, y0, x1, y1;
    footprint_rect(w, h, x0, y0, x1, y1);
    hipLaunchKernelGGL(k_bird_ingest, dim3((w + 255) / 256, h, nframes + nmasks), dim3(256), 0, b->stream, b->d_geom.get(),
                       d_imgs, stride, frame_pitch, d_masks, mask_stride, mask_frame_pitch, b->d_pyr.get(), b->d_mpyr.get(), nframes,
                       b->fpitch(), x0, y0, x1, y1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error("k_bird_ingest", e), ORB_ERR_HIP;
    return bird_body(b, fn, nframes, nmasks, false, kps, desc, cap, counts);
}

extern "C" int orb_bird_extract_batch(orb_bird* b, int nframes, const uint8_t* const* imgs, int w, int h, size_t stride,
                                      const uint8_t* const* masks, int nmasks, size_t mask_stride, orb_keypoint* kps,
                                      uint8_t* desc, int cap, int* counts) {
    static const char* fn = "orb_bird_extract_batch";
    int r;
    bool done;
    if (nframes >= 0 && nmasks != 0 && nmasks != 1 && nmasks != nframes)
        return set_error("orb_bird_extract_batch: nmasks must be 0, 1 or nframes", hipSuccess), ORB_ERR_ARG;
    if (nframes > 0 && nframes <= ORB_BIRD_MAX_BATCH && w > 0 && h > 0) {
        if (nmasks && !masks) return set_error("orb_bird_extract_batch: NULL masks", hipSuccess), ORB_ERR_ARG;
        for (int f = 0; imgs && f < nframes; f++)
            if (!imgs[f]) return set_error("orb_bird_extract_batch: NULL image", hipSuccess), ORB_ERR_ARG;
        for (int m = 0; m < nmasks; m++)
            if (!masks[m]) return set_error("orb_bird_extract_batch: NULL mask", hipSuccess), ORB_ERR_ARG;
    }
    if ((r = bird_frames_enter(b, fn, nframes, imgs, w, h, stride, stride * (size_t)(h > 0 ? h : 0), nmasks > 0, mask_stride,
                               0, kps, desc, true, cap, counts, &done)) != ORB_OK ||
        done)
        return r;
    if ((r = bird_reserve(b, nframes, w, h, nmasks)) != ORB_OK) return r;
    for (int f = 0; f < nframes; f++)
        if ((r = b->upload(imgs[f], stride, nullptr, 0, false, false, f, 0)) != ORB_OK) return r;
    for (int m = 0; m < nmasks; m++)
        if ((r = b->upload(nullptr, 0, masks[m], mask_stride, true, false, 0, m)) != ORB_OK) return r;
    return bird_body(b, fn, nframes, nmasks, false, kps, desc, cap, counts);
}

extern "C" int orb_bird_batch_group(orb_bird* b, int group) {
    if (!b) return set_error("NULL orb_bird", hipSuccess), ORB_ERR_ARG;
    if (group > 0) b->batch_group = std::min(group, ORB_BIRD_MAX_BATCH);
    return b->batch_group;
}

extern "C" int orb_bird_compute(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, orb_keypoint* kps,
                                int* n, uint8_t* desc) {
    int r;
    if ((r = bird_enter(b)) != ORB_OK) return r;
    if (!n || *n < 0 || (*n && !kps)) return set_error("orb_bird_compute: bad arguments", hipSuccess), ORB_ERR_ARG;
    if (!img || w <= 0 || h <= 0) return ORB_OK;   // Feature2D::compute: empty image -> descriptors released
    if (stride < (size_t)w) return ORB_ERR_ARG;
    // detectAndCompute(useProvidedKeypoints): nLevels = max octave + 1; border cull; level sort
    const int n0 = *n;
    int nl = 0;
    bool sorted = true;
    for (int i = 0; i < n0; i++) {
        if (kps[i].octave < 0 || kps[i].octave >= ORBGPU_MAX_LEVELS)
            return set_error("orb_bird_compute: octave out of range", hipSuccess), ORB_ERR_ARG;
        if (i > 0 && kps[i].octave < kps[i - 1].octave) sorted = false;
        nl = std::max(nl, kps[i].octave);
    }
    nl++;
    const int e = b->edge;
    std::vector<orb_keypoint> v;
    v.reserve(n0);
    if (!(h <= 2 * e || w <= 2 * e))
        for (int i = 0; i < n0; i++) {
            const int px = cv_round(kps[i].x), py = cv_round(kps[i].y);
            if (e <= px && px < w - e && e <= py && py < h - e) v.push_back(kps[i]);
        }
    if (!sorted) {
        std::vector<orb_keypoint> s;
        s.reserve(v.size());
        for (int l = 0; l < nl; l++)
            for (const auto& k : v)
                if (k.octave == l) s.push_back(k);
        v.swap(s);
    }
    const int m = (int)v.size();
    std::memcpy(kps, v.data(), m * sizeof(orb_keypoint));
    *n = m;
    if (!m) return ORB_OK;
    if (!desc) return set_error("orb_bird_compute: NULL desc", hipSuccess), ORB_ERR_ARG;
    if ((r = b->ensure_geometry(w, h, std::max(nl, b->nlevels))) != ORB_OK) return r;
    if ((r = b->ensure_kp(m)) != ORB_OK) return r;
    if ((r = b->upload(img, stride, nullptr, 0, false, false)) != ORB_OK) return r;
    if ((r = b->build_pyramid(nl, false)) != ORB_OK) return r;
    hipError_t he;
    if ((he = hipMemcpyAsync(b->d_kps.get(), v.data(), m * sizeof(orb_keypoint), hipMemcpyHostToDevice, b->stream)) !=
        hipSuccess)
        return set_error("birdview keypoint upload", he), ORB_ERR_HIP;
    if ((r = b->launch_blur(nl)) != ORB_OK || (r = b->launch_desc(0, m, false, nullptr)) != ORB_OK) return r;
    if ((he = hipMemcpyAsync(desc, b->d_desc.get(), (size_t)m * 32, hipMemcpyDeviceToHost, b->stream)) != hipSuccess ||
        (he = hipStreamSynchronize(b->stream)) != hipSuccess)
        return set_error("birdview descriptor download", he), ORB_ERR_HIP;
    return ORB_OK;
}

extern "C" int orb_corner_subpix(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, float* pts, int n,
                                 int win_w, int win_h, int max_iter, double eps) {
    int r;
    if ((r = bird_enter(b)) != ORB_OK) return r;
    if (n < 0 || (n && !pts) || !img || w <= 0 || h <= 0 || stride < (size_t)w)
        return set_error("orb_corner_subpix: bad arguments", hipSuccess), ORB_ERR_ARG;
    if (win_w != kSubWin || win_h != kSubWin)   // the kernel is built for the reference's Size(5,5)
        return set_error("orb_corner_subpix: only win (5,5) is built (Frame.cc:337)", hipSuccess), ORB_ERR_ARG;
    if (w < kSubWin * 2 + 5 || h < kSubWin * 2 + 5) return ORB_ERR_GEOMETRY;   // CV_Assert in cornerSubPix
    if (!n) return ORB_OK;
    if ((r = b->ensure_geometry(w, h, b->nlevels)) != ORB_OK && (r = b->ensure_geometry(w, h, 1)) != ORB_OK) return r;
    hipError_t e;
    if ((e = b->d_pts.ensure((size_t)n * 2)) != hipSuccess) return set_error("subpix points", e), ORB_ERR_NOMEM;
    if ((r = b->upload(img, stride, nullptr, 0, false, false)) != ORB_OK) return r;
    const int iters = std::min(std::max(max_iter, 1), 100);
    const double ep = std::max(eps, 0.);
    SubpixSrc s{b->d_pyr.get() + b->g.L[0].off, b->g.L[0].pitch, w, h};
    if ((e = hipMemcpyAsync(b->d_pts.get(), pts, (size_t)n * 8, hipMemcpyHostToDevice, b->stream)) != hipSuccess)
        return set_error("subpix upload", e), ORB_ERR_HIP;
    hipLaunchKernelGGL(k_bird_subpix, dim3((n + 3) / 4), dim3(256), 0, b->stream, s, b->d_wmask.get(), b->d_pts.get(), 2, n, iters,
                       ep * ep, b->edge, (int*)nullptr, (const int*)nullptr, 0u);
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipMemcpyAsync(pts, b->d_pts.get(), (size_t)n * 8, hipMemcpyDeviceToHost, b->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(b->stream)) != hipSuccess)
        return set_error("k_bird_subpix", e), ORB_ERR_HIP;
    return ORB_OK;
}

extern "C" int orb_bird_debug_candidates(orb_bird* b, int level, orb_keypoint* out, int cap) {
    if (!b || level < 0 || level >= (int)b->last_lvlcnt.size()) return ORB_ERR_ARG;
    size_t off = 0;
    for (int l = 0; l < level; l++) off += b->last_lvlcnt[l];
    const int n = b->last_lvlcnt[level];
    if (n > cap) return -n - 1;
    for (int i = 0; i < n; i++) {
        const BirdCand& c = b->last_cands[off + i];
        out[i] = {(float)(c.xy & 0xFFFF), (float)(c.xy >> 16), 7.f, -1.f, c.harris, level, c.score};
    }
    return n;
}

extern "C" int orb_bird_debug_level(orb_bird* b, int level, uint8_t* out, int* w, int* h) {
    if (!b || level < 0 || !b->have_geom || level >= b->g.nlevels || !w || !h) return ORB_ERR_ARG;
    const BirdLevel& L = b->g.L[level];
    *w = L.w;
    *h = L.h;
    if (!out) return ORB_OK;
    (void)hipSetDevice(b->device);
    hipError_t e = hipMemcpy2DAsync(out, L.w, b->d_pyr.get() + L.off, L.pitch, L.w, L.h, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    return e == hipSuccess ? ORB_OK : (set_error("orb_bird_debug_level", e), ORB_ERR_HIP);
}
