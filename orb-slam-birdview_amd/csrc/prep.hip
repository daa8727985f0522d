// The mono_fisheye driver's input (Examples/Monocular/mono_fisheye.cc:94-116): applyMask, the crop, the half-size
// cv::resize and the cvtColor of Tracking::GrabImageMonocularWithBirdview (Tracking.cc:278-307) as one pass over the
// camera frame (k_front_prep), and ConvertMaskBirdview (:244-271) for the per-frame birdview mask (k_bird_mask).  Both
// have exact integer definitions (prep_def.h), restated once for the host twins and the kernels.  Both kernels are
// HBM-bound: k_front_prep reads cw * ch * C source bytes and writes cw * ch / 4; the mask is per camera and resident.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "prep.h"

namespace orbgpu {

constexpr int kPrepThreads = 256;

// Eight source pixels of one row as dwords.  aligned(4): the row base is only known to be dword aligned, and global
// loads of 2, 4 or 6 dwords need no more on gfx950.
template <int C>
struct __attribute__((aligned(4))) PrepRow {
    uint32_t v[2 * C];
};

// get() of prep_def.h over the registers of the wide path: the block of output pixel k of the lane
template <int C>
struct PrepWords {
    const uint32_t* r0;
    const uint32_t* r1;
    int k;
    __device__ uint32_t operator()(int r, int i) const {
        const int j = 2 * C * k + i;
        return ((r ? r1 : r0)[j >> 2] >> ((j & 3) * 8)) & 255u;
    }
};

// Four output pixels per lane: lane q of output row r produces pixels [4 q, 4 q + 4) from source pixels [8 q, 8 q + 8)
// of the crop's rows 2 r and 2 r + 1: 8 C bytes from each row (C = 1: one dwordx2; C = 3: dwordx4 + dwordx2; C = 4: two
// dwordx4) and one 16-bit word of the keep plane, into one dword store.  A wave covers 512 contiguous source pixels of
// two rows and 256 contiguous destination bytes.  Lanes are laid over (row, quad) of one frame without a gap, frames go
// over blockIdx.y (strided: the grid's y is capped); the keep word is loaded once for all of a lane's frames.  The
// wide path needs both source rows at the crop's first column (src is already there: base + cy * stride + cx * C) and
// the destination row base dword aligned, and all four pixels inside the row; every other lane (unaligned bases, odd
// strides, an odd cx * C, the last quad of a row whose width is no multiple of 4) goes byte by byte.  No lane reads
// outside the crop rows' [cx * C, (cx + cw) * C) or writes outside [row, row + cw / 2).
template <int C>
__global__ __launch_bounds__(kPrepThreads) void k_front_prep(const uint8_t* __restrict__ src,
                                                             const uint16_t* __restrict__ keep,
                                                             uint8_t* __restrict__ dst, int nframes, unsigned ow,
                                                             unsigned oh, unsigned quads, size_t src_fp, size_t src_rs,
                                                             size_t dst_fp, size_t dst_rs, uint32_t w0, uint32_t w2) {
    const unsigned id = blockIdx.x * kPrepThreads + threadIdx.x;
    const unsigned row = id / quads;
    if (row >= oh) return;
    const unsigned x0 = (id - row * quads) * 4u;
    const uint32_t kq = keep ? keep[id] : 0xFFFFu;   // (id = row * quads + quad: the plane's own order)
    for (int f = blockIdx.y; f < nframes; f += gridDim.y) {
        const uint8_t* s0 = src + (size_t)f * src_fp + (size_t)(2u * row) * src_rs;
        const uint8_t* s1 = s0 + src_rs;
        uint8_t* d = dst + (size_t)f * dst_fp + (size_t)row * dst_rs;
        const bool aligned = ((reinterpret_cast<uintptr_t>(s0) | reinterpret_cast<uintptr_t>(s1) |
                               reinterpret_cast<uintptr_t>(d)) & 3u) == 0;
        if (aligned && x0 + 4u <= ow) {
            const PrepRow<C> a = *reinterpret_cast<const PrepRow<C>*>(s0 + (size_t)x0 * (2 * C));
            const PrepRow<C> b = *reinterpret_cast<const PrepRow<C>*>(s1 + (size_t)x0 * (2 * C));
            uint32_t y = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                y |= prep_pixel<C>(PrepWords<C>{a.v, b.v, k}, (kq >> (4 * k)) & 15u, w0, w2) << (8 * k);
            *reinterpret_cast<uint32_t*>(d + x0) = y;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned x = x0 + (unsigned)k;
                if (x < ow)
                    d[x] = (uint8_t)prep_pixel<C>(PrepBytes{s0 + (size_t)x * (2 * C), s1 + (size_t)x * (2 * C)},
                                                  (kq >> (4 * k)) & 15u, w0, w2);
            }
        }
    }
}

hipError_t launch_front_prep(const orb_prep& p, int code, const uint8_t* d_crop, int nframes, size_t src_frame_pitch,
                             size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch, size_t dst_row_stride,
                             hipStream_t stream) {
    uint32_t w0, w2;
    gray_weights(code, w0, w2);
    const unsigned ow = (unsigned)p.cw / 2u, oh = (unsigned)p.ch / 2u, quads = (unsigned)p.quads;
    const unsigned lanes = quads * oh;   // <= 1,024 * 4,096
    const dim3 grid((lanes + kPrepThreads - 1) / kPrepThreads, (unsigned)std::min(nframes, 65535));
    const uint16_t* keep = p.d_keep.get();
    switch (prep_channels(code)) {
        case 1:
            hipLaunchKernelGGL(k_front_prep<1>, grid, dim3(kPrepThreads), 0, stream, d_crop, keep, d_dst, nframes, ow, oh,
                               quads, src_frame_pitch, src_row_stride, dst_frame_pitch, dst_row_stride, w0, w2);
            break;
        case 3:
            hipLaunchKernelGGL(k_front_prep<3>, grid, dim3(kPrepThreads), 0, stream, d_crop, keep, d_dst, nframes, ow, oh,
                               quads, src_frame_pitch, src_row_stride, dst_frame_pitch, dst_row_stride, w0, w2);
            break;
        default:
            hipLaunchKernelGGL(k_front_prep<4>, grid, dim3(kPrepThreads), 0, stream, d_crop, keep, d_dst, nframes, ow, oh,
                               quads, src_frame_pitch, src_row_stride, dst_frame_pitch, dst_row_stride, w0, w2);
    }
    return hipGetLastError();
}

// ---- ConvertMaskBirdview ----

template <int C>
struct __attribute__((aligned(4))) MaskQuad {
    uint32_t v[C];
};

// Four mask pixels per lane, as k_to_gray lays them: 12 or 16 source bytes (one dwordx3 / dwordx4 load) into one dword
// store where both row bases are dword aligned and the quad lies inside the row, byte by byte everywhere else.  A pixel
// inside the footprint [fx0, fx1) x [fy0, fy1) is 0.  No lane reads outside [row, row + w * C) or writes outside
// [row, row + w).
template <int C>
__global__ __launch_bounds__(kPrepThreads) void k_bird_mask(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            int nframes, unsigned w, unsigned h, unsigned quads,
                                                            size_t src_fp, size_t src_rs, size_t dst_fp, size_t dst_rs,
                                                            unsigned fx0, unsigned fy0, unsigned fx1, unsigned fy1) {
    const unsigned id = blockIdx.x * kPrepThreads + threadIdx.x;
    const unsigned row = id / quads;
    if (row >= h) return;
    const unsigned x0 = (id - row * quads) * 4u;
    const bool frow = row >= fy0 && row < fy1;
    for (int f = blockIdx.y; f < nframes; f += gridDim.y) {
        const uint8_t* s = src + (size_t)f * src_fp + (size_t)row * src_rs;
        uint8_t* d = dst + (size_t)f * dst_fp + (size_t)row * dst_rs;
        const bool aligned = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 3u) == 0;
        if (aligned && x0 + 4u <= w) {
            const MaskQuad<C> q = *reinterpret_cast<const MaskQuad<C>*>(s + (size_t)x0 * C);
            uint32_t g[4];
            if constexpr (C == 3) {   // G is byte 1, 4, 7, 10 of three dwords
                g[0] = (q.v[0] >> 8) & 255u;
                g[1] = q.v[1] & 255u;
                g[2] = q.v[1] >> 24;
                g[3] = (q.v[2] >> 16) & 255u;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) g[k] = (q.v[k] >> 8) & 255u;
            }
            uint32_t y = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned x = x0 + (unsigned)k;
                const uint32_t v = (frow && x >= fx0 && x < fx1) ? 0u : bird_mask_value(g[k]);
                y |= v << (8 * k);
            }
            *reinterpret_cast<uint32_t*>(d + x0) = y;
        } else {
            const unsigned x1 = x0 + 4u < w ? x0 + 4u : w;
            for (unsigned x = x0; x < x1; x++)
                d[x] = (frow && x >= fx0 && x < fx1) ? (uint8_t)0 : (uint8_t)bird_mask_value(s[(size_t)x * C + 1]);
        }
    }
}

namespace {

constexpr int kMaxSourceSide = 8192;   // the output side stays within the extractor's 4096
constexpr int kMaxMaskSide = 4096;

// The footprint's rectangle at w x h, read off orb_bird_footprint_mask itself: bird.hip keeps the one statement of the
// rectangle, and the kernel needs its four numbers.  One size is remembered (a stream of masks has one size).
struct FootRect {
    int w = -1, h = -1;
    unsigned x0 = 0, y0 = 0, x1 = 0, y1 = 0;
};

bool footprint_of(int w, int h, FootRect& out) {
    static std::mutex mu;
    static FootRect last;
    std::lock_guard<std::mutex> lock(mu);
    if (last.w != w || last.h != h) {
        std::vector<uint8_t> m;
        try {
            m.assign((size_t)w * (size_t)h, 1);
        } catch (const std::bad_alloc&) {
            return false;
        }
        if (orb_bird_footprint_mask(m.data(), w, h, (size_t)w) != ORB_OK) return false;
        FootRect r;
        r.w = w;
        r.h = h;
        for (int y = 0; y < h; y++) {
            const uint8_t* row = m.data() + (size_t)y * w;
            const uint8_t* z = static_cast<const uint8_t*>(std::memchr(row, 0, (size_t)w));
            if (!z) continue;
            if (r.y1 == 0) {   // the first footprint row gives the columns
                r.y0 = (unsigned)y;
                r.x0 = (unsigned)(z - row);
                r.x1 = r.x0;
                while (r.x1 < (unsigned)w && row[r.x1] == 0) r.x1++;
            }
            r.y1 = (unsigned)y + 1;
        }
        last = r;
    }
    out = last;
    return true;
}

// The source, mask and crop of the front-image entry points (the crop is the handle's where there is one).  nullptr,
// or why the call is refused.  A destination is checked with check_dst.
const char* prep_fault(int code, int nframes, int sw, int sh, size_t src_fp, size_t src_rs, bool with_mask,
                       int mask_channels, size_t mask_stride, int cx, int cy, int cw, int ch, size_t dst_fp,
                       size_t dst_rs, bool check_src, bool check_dst) {
    const int C = prep_channels(code);
    if (!C) return "unknown code (ORB_PREP_GRAY or an ORB_COLOR_* code expected)";
    if (with_mask && mask_channels != 1 && mask_channels != 3) return "mask_channels not 1 or 3";
    if (sw < 0 || sh < 0 || nframes < 0) return "negative size";
    if (cx < 0 || cy < 0 || cw < 0 || ch < 0) return "negative crop";
    if ((cw | ch) & 1) return "odd crop side (the half-size resize is then no 2x2 mean)";
    if (sw > kMaxSourceSide || sh > kMaxSourceSide) return "a source side above 8192";
    if ((long long)cx + cw > sw || (long long)cy + ch > sh) return "crop outside the source";
    if (with_mask && mask_stride < (size_t)sw * (size_t)mask_channels) return "mask stride below sw * mask_channels";
    if (nframes == 0 || cw == 0 || ch == 0) return nullptr;
    if (check_src && src_rs < (size_t)sw * C) return "source stride below sw * channels";
    if (check_dst && dst_rs < (size_t)cw / 2) return "destination stride below cw / 2";
    if (nframes > 1) {
        if (check_src && src_fp < (size_t)(sh - 1) * src_rs + (size_t)sw * C)
            return "source frame pitch below a frame's bytes";
        if (check_dst && dst_fp < (size_t)(ch / 2 - 1) * dst_rs + (size_t)cw / 2)
            return "destination frame pitch below a frame's bytes";
    }
    return nullptr;
}

const char* prep_handle_fault(const orb_prep* p, const Ctx* c) {
    if (!p) return "prep NULL";
    if (c && p->device != c->device) return "the handle lives on another device";
    return nullptr;
}

const char* bird_mask_fault(int channels, int nframes, int w, int h, size_t src_fp, size_t src_rs, size_t dst_fp,
                            size_t dst_rs) {
    if (channels != 3 && channels != 4) return "channels not 3 or 4";
    if (w < 0 || h < 0 || nframes < 0) return "negative size";
    if (w > kMaxMaskSide || h > kMaxMaskSide) return "a side above 4096";
    if (w == 0 || h == 0 || nframes == 0) return nullptr;
    if (src_rs < (size_t)w * channels) return "source stride below w * channels";
    if (dst_rs < (size_t)w) return "destination stride below w";
    if (nframes > 1) {
        if (src_fp < (size_t)(h - 1) * src_rs + (size_t)w * channels) return "source frame pitch below a frame's bytes";
        if (dst_fp < (size_t)(h - 1) * dst_rs + (size_t)w) return "destination frame pitch below a frame's bytes";
    }
    return nullptr;
}

}  // namespace
}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_front_prep_host(int code, const uint8_t* src, int sw, int sh, size_t src_stride, const uint8_t* mask,
                        int mask_channels, size_t mask_stride, int cx, int cy, int cw, int ch, uint8_t* dst,
                        size_t dst_stride) {
    const char* const fn = "orb_front_prep_host";
    if (const char* why = prep_fault(code, 1, sw, sh, 0, src_stride, mask != nullptr, mask_channels, mask_stride, cx, cy,
                                     cw, ch, 0, dst_stride, true, true))
        return arg_error(fn, why);
    if (cw == 0 || ch == 0) return ORB_OK;
    if (!src || !dst) return arg_error(fn, "NULL arrays with a non-empty crop");
    uint32_t w0, w2;
    gray_weights(code, w0, w2);
    switch (prep_channels(code)) {
        case 1:
            front_prep_image_host<1>(src, src_stride, mask, mask_channels, mask_stride, cx, cy, cw, ch, w0, w2, dst,
                                     dst_stride);
            break;
        case 3:
            front_prep_image_host<3>(src, src_stride, mask, mask_channels, mask_stride, cx, cy, cw, ch, w0, w2, dst,
                                     dst_stride);
            break;
        default:
            front_prep_image_host<4>(src, src_stride, mask, mask_channels, mask_stride, cx, cy, cw, ch, w0, w2, dst,
                                     dst_stride);
    }
    return ORB_OK;
}

int orb_prep_create(orb_ctx* h, int sw, int sh, const uint8_t* mask, int mask_channels, size_t mask_stride, int cx,
                    int cy, int cw, int ch, orb_prep** out) {
    const char* const fn = "orb_prep_create";
    if (!out) return arg_error(fn, "out NULL");
    if (const char* why = prep_fault(ORB_PREP_GRAY, 1, sw, sh, 0, 0, mask != nullptr, mask_channels, mask_stride, cx, cy,
                                     cw, ch, 0, 0, false, false))
        return arg_error(fn, why);
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    orb_prep* p = new (std::nothrow) orb_prep();
    if (!p) return set_error("orb_prep", hipSuccess), ORB_ERR_NOMEM;
    p->device = c->device;
    p->sw = sw;
    p->sh = sh;
    p->cx = cx;
    p->cy = cy;
    p->cw = cw;
    p->ch = ch;
    p->quads = (cw / 2 + 3) / 4;
    const size_t words = (size_t)p->quads * (size_t)(ch / 2);
    if (words == 0 || !mask) {   // an empty crop: every call through it is ORB_OK with nothing touched; no mask: no plane
        *out = p;
        return ORB_OK;
    }
    std::vector<uint16_t> host;
    try {
        host.assign(words, 0);
    } catch (const std::bad_alloc&) {
        delete p;
        return set_error("orb_prep host staging", hipSuccess), ORB_ERR_NOMEM;
    }
    prep_keep_plane(mask, mask_channels, mask_stride, cx, cy, cw, ch, host.data());
    hipError_t e;
    if ((e = p->d_keep.ensure(words)) != hipSuccess) {
        delete p;
        return set_error("orb_prep allocation", e), ORB_ERR_NOMEM;
    }
    if ((e = hipMemcpyAsync(p->d_keep.get(), host.data(), words * 2, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        delete p;
        return set_error("orb_prep upload", e), ORB_ERR_HIP;
    }
    *out = p;
    return ORB_OK;
}

void orb_prep_destroy(orb_prep* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);   // (as orb_rectify_destroy)
    delete p;
}

int orb_prep_size(const orb_prep* p, int* w, int* h) {
    if (!p || !w || !h) return arg_error("orb_prep_size", "NULL argument");
    *w = p->cw / 2;
    *h = p->ch / 2;
    return ORB_OK;
}

int orb_prep_source_size(const orb_prep* p, int* sw, int* sh) {
    if (!p || !sw || !sh) return arg_error("orb_prep_source_size", "NULL argument");
    *sw = p->sw;
    *sh = p->sh;
    return ORB_OK;
}

int orb_front_prep_device(orb_ctx* h, const orb_prep* p, int code, const uint8_t* d_src, int nframes,
                          size_t src_frame_pitch, size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch,
                          size_t dst_row_stride) {
    const char* const fn = "orb_front_prep_device";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const char* why = prep_handle_fault(p, c)) return arg_error(fn, why);
    if (const char* why = prep_fault(code, nframes, p->sw, p->sh, src_frame_pitch, src_row_stride, false, 0, 0, p->cx,
                                     p->cy, p->cw, p->ch, dst_frame_pitch, dst_row_stride, true, true))
        return arg_error(fn, why);
    if (nframes == 0 || p->cw == 0 || p->ch == 0) return ORB_OK;
    if (!d_src || !d_dst) return arg_error(fn, "NULL arrays with a non-empty crop");
    CTX_GUARD(c);
    const uint8_t* d_crop = d_src + (size_t)p->cy * src_row_stride + (size_t)p->cx * prep_channels(code);
    const hipError_t e = launch_front_prep(*p, code, d_crop, nframes, src_frame_pitch, src_row_stride, d_dst,
                                           dst_frame_pitch, dst_row_stride, c->stream);
    if (e != hipSuccess) return set_error("k_front_prep", e), ORB_ERR_HIP;
    return ORB_OK;
}

int orb_extract_fisheye(orb_ctx* h, const orb_prep* p, int code, const uint8_t* img, size_t stride, orb_keypoint* kps,
                        int cap, int* n, uint8_t* desc) {
    const char* const fn = "orb_extract_fisheye";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const char* why = prep_handle_fault(p, c)) return arg_error(fn, why);
    // (an empty image is judged first by its size: a NULL image of a positive size is orb_extract's empty image too)
    if (const char* why = prep_fault(code, 1, p->sw, p->sh, 0, img ? stride : (size_t)-1, false, 0, 0, p->cx, p->cy,
                                     p->cw, p->ch, 0, 0, true, false))
        return arg_error(fn, why);
    CTX_GUARD(c);
    // _image.empty(), before or after the crop: outputs untouched (ORBextractor.cc:1046-1047)
    if (!img || p->cw == 0 || p->ch == 0) return ORB_OK;
    if (!n) return arg_error(fn, "n NULL");
    // the single-frame chain with the crop's upload and k_front_prep in place of the gray upload; its image is the
    // prepared one, cw / 2 x ch / 2
    return extract_host(c, HostImage{img, p->sw, p->sh, stride, code, nullptr, p}, kps, cap, n, desc);
}

int orb_bird_mask_host(int channels, const uint8_t* src, int w, int h, size_t src_stride, uint8_t* dst,
                       size_t dst_stride) {
    const char* const fn = "orb_bird_mask_host";
    if (const char* why = bird_mask_fault(channels, 1, w, h, 0, src_stride, 0, dst_stride)) return arg_error(fn, why);
    if (w == 0 || h == 0) return ORB_OK;
    if (!src || !dst) return arg_error(fn, "NULL arrays with a non-empty mask");
    bird_mask_convert_host(channels, src, w, h, src_stride, dst, dst_stride);
    return orb_bird_footprint_mask(dst, w, h, dst_stride);   // the one statement of the rectangle (bird.hip)
}

int orb_bird_mask_device(orb_ctx* h, int channels, const uint8_t* d_src, int nframes, int w, int hgt,
                         size_t src_frame_pitch, size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch,
                         size_t dst_row_stride) {
    const char* const fn = "orb_bird_mask_device";
    if (const char* why = bird_mask_fault(channels, nframes, w, hgt, src_frame_pitch, src_row_stride, dst_frame_pitch,
                                          dst_row_stride))
        return arg_error(fn, why);
    if (nframes == 0 || w == 0 || hgt == 0) return ORB_OK;
    if (!d_src || !d_dst) return arg_error(fn, "NULL arrays with a non-empty mask");
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    FootRect r;
    if (!footprint_of(w, hgt, r)) return set_error("orb_bird_mask_device: footprint staging", hipSuccess), ORB_ERR_NOMEM;
    const unsigned quads = ((unsigned)w + 3u) / 4u;
    const unsigned lanes = quads * (unsigned)hgt;   // <= 1,024 * 4,096
    const dim3 grid((lanes + kPrepThreads - 1) / kPrepThreads, (unsigned)std::min(nframes, 65535));
    if (channels == 3)
        hipLaunchKernelGGL(k_bird_mask<3>, grid, dim3(kPrepThreads), 0, c->stream, d_src, d_dst, nframes, (unsigned)w,
                           (unsigned)hgt, quads, src_frame_pitch, src_row_stride, dst_frame_pitch, dst_row_stride, r.x0,
                           r.y0, r.x1, r.y1);
    else
        hipLaunchKernelGGL(k_bird_mask<4>, grid, dim3(kPrepThreads), 0, c->stream, d_src, d_dst, nframes, (unsigned)w,
                           (unsigned)hgt, quads, src_frame_pitch, src_row_stride, dst_frame_pitch, dst_row_stride, r.x0,
                           r.y0, r.x1, r.y1);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error("k_bird_mask", e), ORB_ERR_HIP;
    return ORB_OK;
}

}  // extern "C"
