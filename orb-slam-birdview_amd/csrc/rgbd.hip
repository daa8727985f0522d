// Colour input and the RGB-D constructor: cvtColor to gray as Tracking::GrabImage* opens (Tracking.cc:172-307) and
// Frame::ComputeStereoFromRGBD (Frame.cc:839-860) with GrabImageRGBD's convertTo folded in (Tracking.cc:229-230).
// Both have exact definitions (an integer formula; two float operations), restated once for the host twins and the
// kernels: k_to_gray (HBM-bound: 3 or 4 bytes in, 1 byte out per pixel) and k_rgbd_depth (a gather, launch-bound).
#include <climits>
#include <cmath>

#include "gray_def.h"
#include "rgbd.h"
#include "undistort.h"

namespace orbgpu {

// (gray_of and gray_weights, the cvtColor definition: gray_def.h)

constexpr int kGrayThreads = 256;

// Four pixels of source as dwords.  aligned(4): the row base is only known to be dword aligned, and global loads of
// 3 or 4 dwords need no more on gfx950.
template <int C>
struct __attribute__((aligned(4))) GrayQuad {
    uint32_t v[C];
};

// Four output pixels per lane: lane q of row r converts pixels [4 q, 4 q + 4) from 12 or 16 source bytes (one
// dwordx3 / dwordx4 load) into one dword store; a wave covers 768 or 1,024 contiguous source bytes and 256 contiguous
// destination bytes.  Lanes are laid over (row, quad) of one frame without a gap (quads = ceil(w / 4) lanes per row),
// frames go over blockIdx.y (strided: the grid's y is capped).  The dword path needs the source and the destination
// row base dword aligned and all four pixels inside the row; every other lane (a row whose bases are not aligned:
// odd strides, offset bases; the last quad of a row whose width is no multiple of 4) converts its pixels byte by
// byte.  No lane reads outside [row, row + w * C) or writes outside [row, row + w).
template <int C>
__global__ __launch_bounds__(kGrayThreads) void k_to_gray(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          int nframes, unsigned w, unsigned h, unsigned quads,
                                                          size_t src_fp, size_t src_rs, size_t dst_fp, size_t dst_rs,
                                                          uint32_t w0, uint32_t w2) {
    const unsigned id = blockIdx.x * kGrayThreads + threadIdx.x;
    const unsigned row = id / quads;
    if (row >= h) return;
    const unsigned x0 = (id - row * quads) * 4u;
    for (int f = blockIdx.y; f < nframes; f += gridDim.y) {
        const uint8_t* s = src + (size_t)f * src_fp + (size_t)row * src_rs;
        uint8_t* d = dst + (size_t)f * dst_fp + (size_t)row * dst_rs;
        const bool aligned = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 3u) == 0;
        if (aligned && x0 + 4u <= w) {
            const GrayQuad<C> q = *reinterpret_cast<const GrayQuad<C>*>(s + (size_t)x0 * C);
            uint32_t y0, y1, y2, y3;
            if constexpr (C == 3) {   // bytes 0..11 of three dwords
                const uint32_t a = q.v[0], b = q.v[1], c = q.v[2];
                y0 = gray_of(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u, w0, w2);
                y1 = gray_of(a >> 24, b & 255u, (b >> 8) & 255u, w0, w2);
                y2 = gray_of((b >> 16) & 255u, b >> 24, c & 255u, w0, w2);
                y3 = gray_of((c >> 8) & 255u, (c >> 16) & 255u, c >> 24, w0, w2);
            } else {        // one dword per pixel, its fourth byte (alpha) ignored
                y0 = gray_of(q.v[0] & 255u, (q.v[0] >> 8) & 255u, (q.v[0] >> 16) & 255u, w0, w2);
                y1 = gray_of(q.v[1] & 255u, (q.v[1] >> 8) & 255u, (q.v[1] >> 16) & 255u, w0, w2);
                y2 = gray_of(q.v[2] & 255u, (q.v[2] >> 8) & 255u, (q.v[2] >> 16) & 255u, w0, w2);
                y3 = gray_of(q.v[3] & 255u, (q.v[3] >> 8) & 255u, (q.v[3] >> 16) & 255u, w0, w2);
            }
            *reinterpret_cast<uint32_t*>(d + x0) = y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
        } else {
            const unsigned x1 = x0 + 4u < w ? x0 + 4u : w;
            for (unsigned x = x0; x < x1; x++) {
                const uint8_t* p = s + (size_t)x * C;
                d[x] = (uint8_t)gray_of(p[0], p[1], p[2], w0, w2);
            }
        }
    }
}

hipError_t launch_to_gray(int code, const uint8_t* d_src, int nframes, int w, int h, size_t src_frame_pitch,
                          size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch, size_t dst_row_stride,
                          hipStream_t stream) {
    uint32_t w0, w2;
    gray_weights(code, w0, w2);
    const unsigned quads = ((unsigned)w + 3u) / 4u;
    const unsigned lanes = quads * (unsigned)h;   // <= 1,024 * 4,096
    const dim3 grid((lanes + kGrayThreads - 1) / kGrayThreads, (unsigned)std::min(nframes, 65535));
    if (color_channels(code) == 3)
        hipLaunchKernelGGL(k_to_gray<3>, grid, dim3(kGrayThreads), 0, stream, d_src, d_dst, nframes, (unsigned)w,
                           (unsigned)h, quads, src_frame_pitch, src_row_stride, dst_frame_pitch, dst_row_stride, w0, w2);
    else
        hipLaunchKernelGGL(k_to_gray<4>, grid, dim3(kGrayThreads), 0, stream, d_src, d_dst, nframes, (unsigned)w,
                           (unsigned)h, quads, src_frame_pitch, src_row_stride, dst_frame_pitch, dst_row_stride, w0, w2);
    return hipGetLastError();
}

// ---- Frame::ComputeStereoFromRGBD ----

// Mat::at<float>(float, float): the position truncated toward zero.  false: not finite, or outside the image (the
// reference's undefined behaviour; -1 / -1 here).  x in (-1, 0) truncates to column 0 and is inside.
__host__ __device__ inline bool rgbd_locate(float x, float y, int w, int h, int& col, int& row) {
    if (!(x > -1.0f && x < (float)w && y > -1.0f && y < (float)h)) return false;   // (w, h <= 4096: exact floats)
    col = (int)x;
    row = (int)y;
    return true;
}

// convertTo(CV_32F, factor) of the one element the keypoint reads: float work type, beta 0, one rounding
__host__ __device__ inline float rgbd_value(const uint8_t* map, int type, size_t row_stride, int row, int col,
                                            float factor) {
    const uint8_t* p = map + (size_t)row * row_stride;
    const float raw = type == ORB_DEPTH_U16 ? (float)reinterpret_cast<const uint16_t*>(p)[col]
                                            : reinterpret_cast<const float*>(p)[col];
    return raw * factor;
}

constexpr int kDepthThreads = 256;

// One workgroup per frame of a batch in orb_extract_batch_device's output layout; its lanes stride over the frame's
// keypoints (a few thousand at the most), so the frame's count of valid depths is one workgroup reduction and one
// plain store: no atomics, nothing to clear.  The position is checked before the map is read.  raw and un may be the
// same array.  Slots past the frame's count are not touched.
__global__ __launch_bounds__(kDepthThreads) void k_rgbd_depth(const uint8_t* map, int type, int w, int h,
                                                              size_t row_stride, size_t frame_pitch, float factor,
                                                              float mbf, const orb_keypoint* raw, const orb_keypoint* un,
                                                              const int* __restrict__ counts, int kp_cap, float* uright,
                                                              float* depth, int* nvalid) {
    const int f = blockIdx.x;
    int n = counts[f];
    if (n > kp_cap) n = kp_cap;
    const uint8_t* m = map + (size_t)f * frame_pitch;
    const size_t base = (size_t)f * (size_t)kp_cap;
    int valid = 0;
    for (int i = threadIdx.x; i < n; i += kDepthThreads) {
        const size_t r = base + (size_t)i;
        float o_ur = -1.0f, o_d = -1.0f;
        int col, row;
        if (rgbd_locate(raw[r].x, raw[r].y, w, h, col, row)) {
            const float d = rgbd_value(m, type, row_stride, row, col, factor);
            if (d > 0) {
                o_d = d;
                o_ur = un[r].x - mbf / d;
                valid++;
            }
        }
        uright[r] = o_ur;
        depth[r] = o_d;
    }
    if (!nvalid) return;   // (uniform)
    __shared__ int part[kDepthThreads / 64];
    for (int o = 32; o > 0; o >>= 1) valid += __shfl_down(valid, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = valid;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < kDepthThreads / 64; k++) t += part[k];
        nvalid[f] = t;
    }
}

hipError_t launch_rgbd_depth(const orb_depth_map& map, float mbf, int nframes, const orb_keypoint* d_raw,
                             const orb_keypoint* d_un, const int* d_counts, int kp_cap, float* d_uright, float* d_depth,
                             int* d_nvalid, hipStream_t stream) {
    hipLaunchKernelGGL(k_rgbd_depth, dim3((unsigned)nframes), dim3(kDepthThreads), 0, stream,
                       static_cast<const uint8_t*>(map.data), map.type, map.w, map.h, map.row_stride, map.frame_pitch,
                       map.factor, mbf, d_raw, d_un, d_counts, kp_cap, d_uright, d_depth, d_nvalid);
    return hipGetLastError();
}

namespace {

constexpr int kMaxSide = 4096;

// The image checks of the three colour entry points (nframes 1 for a single image).  empty: nothing to convert.
const char* gray_fault(int code, int nframes, int w, int h, size_t src_fp, size_t src_rs, size_t dst_fp, size_t dst_rs,
                       bool check_dst) {
    const int ch = color_channels(code);
    if (!ch) return "unknown colour code";
    if (w < 0 || h < 0 || nframes < 0) return "negative size";
    if (w > kMaxSide || h > kMaxSide) return "a side above 4096";
    if (w == 0 || h == 0 || nframes == 0) return nullptr;
    if (src_rs < (size_t)w * ch) return "source stride below w * channels";
    if (check_dst && dst_rs < (size_t)w) return "destination stride below w";
    if (nframes > 1) {
        if (src_fp < (size_t)(h - 1) * src_rs + (size_t)w * ch) return "source frame pitch below a frame's bytes";
        if (check_dst && dst_fp < (size_t)(h - 1) * dst_rs + (size_t)w)
            return "destination frame pitch below a frame's bytes";
    }
    return nullptr;
}

size_t depth_elem(int type) { return type == ORB_DEPTH_U16 ? 2 : type == ORB_DEPTH_F32 ? 4 : 0; }

const char* depth_fault(const orb_depth_map* m, float mbf, int nframes) {
    if (!m) return "map NULL";
    const size_t es = depth_elem(m->type);
    if (!es) return "unknown depth type";
    if (!std::isfinite(m->factor)) return "factor not finite";
    if (!std::isfinite(mbf)) return "mbf not finite";
    if (m->w < 0 || m->h < 0) return "negative map size";
    if (m->w > kMaxSide || m->h > kMaxSide) return "a map side above 4096";
    if (m->row_stride < (size_t)m->w * es) return "row_stride below w * element size";
    if (nframes > 1 && m->frame_pitch < m->row_stride * (size_t)m->h) return "frame_pitch below row_stride * h";
    if (reinterpret_cast<uintptr_t>(m->data) % es || m->row_stride % es || (nframes > 1 && m->frame_pitch % es))
        return "map not aligned to its element size";
    return nullptr;
}

}  // namespace
}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_to_gray_host(int code, const uint8_t* src, int w, int h, size_t src_stride, uint8_t* dst, size_t dst_stride) {
    const char* const fn = "orb_to_gray_host";
    if (const char* why = gray_fault(code, 1, w, h, 0, src_stride, 0, dst_stride, true)) return arg_error(fn, why);
    if (w == 0 || h == 0) return ORB_OK;
    if (!src || !dst) return arg_error(fn, "NULL arrays with a non-empty image");
    const int ch = color_channels(code);
    uint32_t w0, w2;
    gray_weights(code, w0, w2);
    for (int y = 0; y < h; y++) {
        const uint8_t* s = src + (size_t)y * src_stride;
        uint8_t* d = dst + (size_t)y * dst_stride;
        for (int x = 0; x < w; x++, s += ch) d[x] = (uint8_t)gray_of(s[0], s[1], s[2], w0, w2);
    }
    return ORB_OK;
}

int orb_to_gray_device(orb_ctx* h, int code, const uint8_t* d_src, int nframes, int w, int hgt, size_t src_frame_pitch,
                       size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch, size_t dst_row_stride) {
    const char* const fn = "orb_to_gray_device";
    if (const char* why = gray_fault(code, nframes, w, hgt, src_frame_pitch, src_row_stride, dst_frame_pitch,
                                     dst_row_stride, true))
        return arg_error(fn, why);
    if (nframes == 0 || w == 0 || hgt == 0) return ORB_OK;
    if (!d_src || !d_dst) return arg_error(fn, "NULL arrays with a non-empty image");
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    const hipError_t e = launch_to_gray(code, d_src, nframes, w, hgt, src_frame_pitch, src_row_stride, d_dst,
                                        dst_frame_pitch, dst_row_stride, c->stream);
    if (e != hipSuccess) return set_error("k_to_gray", e), ORB_ERR_HIP;
    return ORB_OK;
}

int orb_extract_color(orb_ctx* h, int code, const uint8_t* img, int w, int hgt, size_t stride, orb_keypoint* kps,
                      int cap, int* n, uint8_t* desc) {
    const char* const fn = "orb_extract_color";
    // (an empty image is judged first by its size: a NULL image of a positive size is orb_extract's empty image too)
    if (const char* why = gray_fault(code, 1, w, hgt, 0, img ? stride : (size_t)-1, 0, 0, false))
        return arg_error(fn, why);
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (!img || w == 0 || hgt == 0) return ORB_OK;   // _image.empty(): outputs untouched (ORBextractor.cc:1046-1047)
    if (!n) return arg_error(fn, "n NULL");
    // the single-frame chain with the colour upload and k_to_gray in place of the gray upload
    return extract_host(c, HostImage{img, w, hgt, stride, code}, kps, cap, n, desc);
}

int orb_stereo_from_rgbd_host(const orb_depth_map* map, float mbf, int n, const orb_keypoint* kps,
                              const orb_keypoint* kps_un, float* uright, float* depth, int* nvalid) {
    const char* const fn = "orb_stereo_from_rgbd_host";
    if (const char* why = depth_fault(map, mbf, 1)) return arg_error(fn, why);
    if (n < 0) return arg_error(fn, "n < 0");
    if (n > 0 && (!map->data || !kps || !kps_un || !uright || !depth)) return arg_error(fn, "NULL arrays with n > 0");
    int col, row;
    for (int i = 0; i < n; i++)
        if (!rgbd_locate(kps[i].x, kps[i].y, map->w, map->h, col, row))
            return arg_error(fn, "a keypoint position is not finite or outside the map");
    const uint8_t* m = static_cast<const uint8_t*>(map->data);
    int valid = 0;
    for (int i = 0; i < n; i++) {
        rgbd_locate(kps[i].x, kps[i].y, map->w, map->h, col, row);
        const float d = rgbd_value(m, map->type, map->row_stride, row, col, map->factor);
        const float xu = kps_un[i].x;   // (read before the stores: the outputs may not alias, but cost nothing)
        if (d > 0) {
            depth[i] = d;
            uright[i] = xu - mbf / d;
            valid++;
        } else {
            depth[i] = -1.0f;
            uright[i] = -1.0f;
        }
    }
    if (nvalid) *nvalid = valid;
    return ORB_OK;
}

int orb_stereo_from_rgbd_device(orb_ctx* h, const orb_depth_map* map, float mbf, int nframes,
                                const orb_keypoint* d_kps_raw, const orb_keypoint* d_kps_un, const int* d_counts,
                                int kp_cap, float* d_uright, float* d_depth, int* d_nvalid) {
    const char* const fn = "orb_stereo_from_rgbd_device";
    if (const char* why = depth_fault(map, mbf, nframes)) return arg_error(fn, why);
    if (const char* why = batch_fault(nframes, kp_cap)) return arg_error(fn, why);
    if (nframes > 0 && (!map->data || !d_kps_raw || !d_kps_un || !d_counts || !d_uright || !d_depth))
        return arg_error(fn, "NULL arrays with nframes > 0");
    if (nframes == 0) return ORB_OK;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    const hipError_t e = launch_rgbd_depth(*map, mbf, nframes, d_kps_raw, d_kps_un, d_counts, kp_cap, d_uright, d_depth,
                                           d_nvalid, c->stream);
    if (e != hipSuccess) return set_error("k_rgbd_depth", e), ORB_ERR_HIP;
    return ORB_OK;
}

int orb_frames_create_from_batch_rgbd(orb_ctx* h, const orb_distortion* dist, const orb_depth_map* map, float mbf,
                                      int nframes, const uint8_t* d_desc, const orb_keypoint* d_kps_raw,
                                      const int* d_counts, int kp_cap, float min_x, float min_y, float inv_w, float inv_h,
                                      float* d_uright, float* d_depth, orb_frame** out) {
    const char* const fn = "orb_frames_create_from_batch_rgbd";
    if (const char* why = distortion_fault(dist)) return arg_error(fn, why);
    if (const char* why = depth_fault(map, mbf, nframes)) return arg_error(fn, why);
    if (const char* why = batch_fault(nframes, kp_cap)) return arg_error(fn, why);
    if (nframes > 0 && (!map->data || !d_desc || !d_kps_raw || !d_counts || !out))
        return arg_error(fn, "NULL arrays with nframes > 0");
    if (const char* why = grid_fault(min_x, min_y, inv_w, inv_h)) return arg_error(fn, why);
    if (nframes == 0) return ORB_OK;
    const DepthStep step{DepthStep::kRgbd, *map, 0.0f, mbf, d_uright, d_depth};
    std::vector<orb_frame*> F((size_t)nframes, nullptr);
    const int st = frames_from_extract(fn, reinterpret_cast<Ctx*>(h), dist, nframes, d_desc, d_kps_raw, d_counts, 0,
                                       kp_cap, nullptr, min_x, min_y, inv_w, inv_h, F.data(), &step);
    if (st == ORB_OK)
        for (int f = 0; f < nframes; f++) out[f] = F[f];
    return st;
}

}  // extern "C"
