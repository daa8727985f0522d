// Stereo rectification: cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) as every stereo frame of the reference goes
// through it (Examples/Stereo/stereo_euroc.cc:136-137) and cv::initUndistortRectifyMap(..., CV_32F, ...) that builds the
// maps (:97-98).  Both have exact definitions (fixed-point integers; double arithmetic in a stated order), restated once
// for the host twins and the kernel: k_remap is a gather (6 map bytes, up to 4 source bytes in, 1 byte out per pixel),
// HBM-bound on the source and the destination; the maps are shared by the frames of a batch and stay in cache.
#include <new>

#include "remap.h"

namespace orbgpu {

constexpr int kRemapThreads = 256;
constexpr int kRemapFramesPerLane = 4;   // a lane's map values serve this many frames where the batch has them

struct RemapMaps {
    const uint32_t* p[kRemapMaxMaps];
};

// Four destination pixels per lane: lane q of row r produces pixels [4 q, 4 q + 4) of its frames.  Its map values are
// one dwordx4 (the four corners, iy << 16 | ix) and one dwordx2 (the four 10-bit fractions) from the resident planes,
// whose rows are padded to whole quads, so both loads are wide and aligned whatever dw and the images' alignment are.
// The 16 taps are byte loads, each behind its own border test (remap_read): neighbouring lanes gather neighbouring
// source bytes, which the vector cache serves.  The store is one dword where the destination row base is dword aligned
// and the quad lies inside the row; every other lane (odd strides, offset bases, the last quad of a row whose width is
// no multiple of 4) stores byte by byte.  No lane reads outside [0, sw) x [0, sh) of its frame or writes outside
// [row, row + dw).
// Lanes are laid over (row, quad) of one frame without a gap; blockIdx.y = g * nmaps + m serves the frames
// m + nmaps * (g + G k), k = 0, 1, ... (G = gridDim.y / nmaps): one map for all of a lane's frames, loaded once.
__global__ __launch_bounds__(kRemapThreads) void k_remap(RemapMaps maps, int nmaps, unsigned mpitch, unsigned plane1,
                                                         const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         int nframes, int sw, int sh, unsigned dw, unsigned dh,
                                                         unsigned quads, size_t src_fp, size_t src_rs, size_t dst_fp,
                                                         size_t dst_rs) {
    const unsigned id = blockIdx.x * kRemapThreads + threadIdx.x;
    const unsigned row = id / quads;
    if (row >= dh) return;
    const unsigned x0 = (id - row * quads) * 4u;
    const int m = (int)(blockIdx.y % (unsigned)nmaps), g = (int)(blockIdx.y / (unsigned)nmaps);
    const int fstep = (int)gridDim.y;   // (a multiple of nmaps)
    const uint32_t* mp = maps.p[m];
    const size_t mo = (size_t)row * mpitch + x0;
    const uint4 cq = *reinterpret_cast<const uint4*>(mp + mo);
    const uint2 fq = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(mp + plane1) + mo);
    const uint32_t corner[4] = {cq.x, cq.y, cq.z, cq.w};
    const uint32_t frac[4] = {fq.x & 0xFFFFu, fq.x >> 16, fq.y & 0xFFFFu, fq.y >> 16};
    for (int f = g * nmaps + m; f < nframes; f += fstep) {
        const uint8_t* s = src + (size_t)f * src_fp;
        uint8_t* d = dst + (size_t)f * dst_fp + (size_t)row * dst_rs;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int ix = (int)(short)(corner[k] & 0xFFFFu), iy = (int)corner[k] >> 16;
            const uint32_t fx = frac[k] & 31u, fy = frac[k] >> 5;
            v[k] = remap_blend(fx, fy, remap_read(s, src_rs, sw, sh, ix, iy), remap_read(s, src_rs, sw, sh, ix + 1, iy),
                               remap_read(s, src_rs, sw, sh, ix, iy + 1), remap_read(s, src_rs, sw, sh, ix + 1, iy + 1));
        }
        if ((reinterpret_cast<uintptr_t>(d) & 3u) == 0 && x0 + 4u <= dw) {
            *reinterpret_cast<uint32_t*>(d + x0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (x0 + (unsigned)k < dw) d[x0 + k] = (uint8_t)v[k];
        }
    }
}

hipError_t launch_remap(int nmaps, const orb_rectify* const* maps, const uint8_t* d_src, int nframes, int sw, int sh,
                        size_t src_frame_pitch, size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch,
                        size_t dst_row_stride, hipStream_t stream) {
    RemapMaps M{};
    for (int i = 0; i < nmaps; i++) M.p[i] = maps[i]->d_map.get();
    const orb_rectify& r = *maps[0];
    const unsigned quads = (unsigned)r.mpitch / 4u;
    const unsigned lanes = quads * (unsigned)r.dh;   // <= 1,024 * 4,096
    // groups of nmaps frames: at most 65,535 / nmaps in the grid's y, each lane serving up to kRemapFramesPerLane of them
    const int per_map = (nframes + nmaps - 1) / nmaps;
    const int G = std::min((per_map + kRemapFramesPerLane - 1) / kRemapFramesPerLane, 65535 / nmaps);
    const dim3 grid((lanes + kRemapThreads - 1) / kRemapThreads, (unsigned)(G * nmaps));
    hipLaunchKernelGGL(k_remap, grid, dim3(kRemapThreads), 0, stream, M, nmaps, (unsigned)r.mpitch,
                       (unsigned)r.mpitch * (unsigned)r.dh, d_src, d_dst, nframes, sw, sh, (unsigned)r.dw, (unsigned)r.dh,
                       quads, src_frame_pitch, src_row_stride, dst_frame_pitch, dst_row_stride);
    return hipGetLastError();
}

namespace {

constexpr int kMaxSide = 4096;

// The float maps of one call (host memory): NULL with a non-empty size, a stride below a row, misalignment
const char* maps_fault(int dw, int dh, const void* map_x, const void* map_y, size_t map_stride) {
    if (dw < 0 || dh < 0) return "negative map size";
    if (dw > kMaxSide || dh > kMaxSide) return "a map side above 4096";
    if (dw == 0 || dh == 0) return nullptr;
    if (!map_x || !map_y) return "NULL maps with a non-empty size";
    if (map_stride < (size_t)dw * 4) return "map stride below dw * 4";
    if (reinterpret_cast<uintptr_t>(map_x) % 4 || reinterpret_cast<uintptr_t>(map_y) % 4 || map_stride % 4)
        return "maps not aligned to 4 bytes";
    return nullptr;
}

// The source and destination images of the remap entry points (nframes 1 for a single image; the destination's
// size is the maps').  check_dst: the call has a caller-side destination.
const char* remap_fault(int nframes, int sw, int sh, int dw, int dh, size_t src_fp, size_t src_rs, size_t dst_fp,
                        size_t dst_rs, bool check_dst) {
    if (sw < 0 || sh < 0 || nframes < 0) return "negative size";
    if (sw > kMaxSide || sh > kMaxSide) return "a side above 4096";
    if (nframes == 0 || dw == 0 || dh == 0) return nullptr;
    if (src_rs < (size_t)sw) return "source stride below sw";
    if (check_dst && dst_rs < (size_t)dw) return "destination stride below the maps' width";
    if (nframes > 1) {
        if (sw > 0 && sh > 0 && src_fp < (size_t)(sh - 1) * src_rs + (size_t)sw)
            return "source frame pitch below a frame's bytes";
        if (check_dst && dst_fp < (size_t)(dh - 1) * dst_rs + (size_t)dw)
            return "destination frame pitch below a frame's bytes";
    }
    return nullptr;
}

// The handles of one call: at least one, none NULL, one size, one device (c's when there is a context)
const char* handles_fault(int nmaps, const orb_rectify* const* maps, const Ctx* c) {
    if (nmaps < 1) return "nmaps < 1";
    if (nmaps > kRemapMaxMaps) return "more than ORB_REMAP_MAX_MAPS maps";
    if (!maps) return "maps NULL";
    for (int i = 0; i < nmaps; i++)
        if (!maps[i]) return "a NULL map";
    for (int i = 0; i < nmaps; i++) {
        if (maps[i]->dw != maps[0]->dw || maps[i]->dh != maps[0]->dh) return "maps of differing size";
        if (maps[i]->device != (c ? c->device : maps[0]->device)) return "a map lives on another device";
    }
    return nullptr;
}

}  // namespace

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_remap_host(const uint8_t* src, int sw, int sh, size_t src_stride, const float* map_x, const float* map_y,
                   size_t map_stride, int dw, int dh, uint8_t* dst, size_t dst_stride) {
    const char* const fn = "orb_remap_host";
    if (const char* why = maps_fault(dw, dh, map_x, map_y, map_stride)) return arg_error(fn, why);
    if (const char* why = remap_fault(1, sw, sh, dw, dh, 0, src_stride, 0, dst_stride, true)) return arg_error(fn, why);
    if (dw == 0 || dh == 0) return ORB_OK;
    if (!dst || (!src && sw > 0 && sh > 0)) return arg_error(fn, "NULL arrays with a non-empty image");
    remap_image_host(src, sw, sh, src_stride, map_x, map_y, map_stride, dw, dh, dst, dst_stride);
    return ORB_OK;
}

int orb_rectify_maps_host(const double* K, const double* D, int nD, const double* R, const double* P33, int w, int h,
                          float* map_x, float* map_y, size_t map_stride) {
    const char* const fn = "orb_rectify_maps_host";
    if (!K || !R || !P33) return arg_error(fn, "K, R or P33 NULL");
    if (nD != 4 && nD != 5 && nD != 8) return arg_error(fn, "4, 5 or 8 distortion coefficients expected");
    if (!D) return arg_error(fn, "D NULL");
    if (const char* why = maps_fault(w, h, map_x, map_y, map_stride)) return arg_error(fn, why);
    if (w == 0 || h == 0) return ORB_OK;
    if (!rectify_maps_build(K, D, nD, R, P33, w, h, map_x, map_y, map_stride)) return arg_error(fn, "P33 * R is singular");
    return ORB_OK;
}

int orb_rectify_create(orb_ctx* h, int dw, int dh, const float* map_x, const float* map_y, size_t map_stride,
                       orb_rectify** out) {
    const char* const fn = "orb_rectify_create";
    if (!out) return arg_error(fn, "out NULL");
    if (const char* why = maps_fault(dw, dh, map_x, map_y, map_stride)) return arg_error(fn, why);
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    orb_rectify* r = new (std::nothrow) orb_rectify();
    if (!r) return set_error("orb_rectify", hipSuccess), ORB_ERR_NOMEM;
    r->device = c->device;
    r->dw = dw;
    r->dh = dh;
    r->mpitch = (dw + 3) & ~3;
    const size_t px = (size_t)r->mpitch * (size_t)dh;
    if (px == 0) {   // an empty map: every remap through it is ORB_OK with nothing touched
        *out = r;
        return ORB_OK;
    }
    // the conversion OpenCV makes per call and per tile, once: plane 0 as dwords, plane 1 as ushorts behind it
    std::vector<uint32_t> host;
    try {
        host.assign(px + px / 2, 0u);
    } catch (const std::bad_alloc&) {
        delete r;
        return set_error("orb_rectify host staging", hipSuccess), ORB_ERR_NOMEM;
    }
    uint16_t* fr = reinterpret_cast<uint16_t*>(host.data() + px);
    for (int y = 0; y < dh; y++) {
        const float* mx = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(map_x) + (size_t)y * map_stride);
        const float* my = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(map_y) + (size_t)y * map_stride);
        for (int x = 0; x < dw; x++) {
            const RemapTap t = remap_tap(mx[x], my[x]);
            host[(size_t)y * r->mpitch + x] = ((uint32_t)t.iy << 16) | ((uint32_t)t.ix & 0xFFFFu);
            fr[(size_t)y * r->mpitch + x] = (uint16_t)t.frac;
        }
    }
    hipError_t e;
    if ((e = r->d_map.ensure(host.size())) != hipSuccess) {
        delete r;
        return set_error("orb_rectify allocation", e), ORB_ERR_NOMEM;
    }
    if ((e = hipMemcpyAsync(r->d_map.get(), host.data(), host.size() * 4, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        delete r;
        return set_error("orb_rectify upload", e), ORB_ERR_HIP;
    }
    *out = r;
    return ORB_OK;
}

void orb_rectify_destroy(orb_rectify* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);   // (as orb_frame_destroy)
    delete r;
}

int orb_rectify_size(const orb_rectify* r, int* w, int* h) {
    if (!r || !w || !h) return arg_error("orb_rectify_size", "NULL argument");
    *w = r->dw;
    *h = r->dh;
    return ORB_OK;
}

int orb_remap_device(orb_ctx* h, int nmaps, const orb_rectify* const* maps, const uint8_t* d_src, int nframes, int sw,
                     int sh, size_t src_frame_pitch, size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch,
                     size_t dst_row_stride) {
    const char* const fn = "orb_remap_device";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const char* why = handles_fault(nmaps, maps, c)) return arg_error(fn, why);
    const int dw = maps[0]->dw, dh = maps[0]->dh;
    if (const char* why = remap_fault(nframes, sw, sh, dw, dh, src_frame_pitch, src_row_stride, dst_frame_pitch,
                                      dst_row_stride, true))
        return arg_error(fn, why);
    if (nframes == 0 || dw == 0 || dh == 0) return ORB_OK;
    if (!d_dst || (!d_src && sw > 0 && sh > 0)) return arg_error(fn, "NULL arrays with a non-empty image");
    CTX_GUARD(c);
    const hipError_t e = launch_remap(nmaps, maps, d_src, nframes, sw, sh, src_frame_pitch, src_row_stride, d_dst,
                                      dst_frame_pitch, dst_row_stride, c->stream);
    if (e != hipSuccess) return set_error("k_remap", e), ORB_ERR_HIP;
    return ORB_OK;
}

int orb_remap(orb_ctx* h, const orb_rectify* rect, const uint8_t* img, int sw, int sh, size_t stride, uint8_t* dst,
              size_t dst_stride) {
    const char* const fn = "orb_remap";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const char* why = handles_fault(1, &rect, c)) return arg_error(fn, why);
    const int dw = rect->dw, dh = rect->dh;
    if (const char* why = remap_fault(1, sw, sh, dw, dh, 0, stride, 0, dst_stride, true)) return arg_error(fn, why);
    if (dw == 0 || dh == 0) return ORB_OK;
    if (!dst || (!img && sw > 0 && sh > 0)) return arg_error(fn, "NULL arrays with a non-empty image");
    CTX_GUARD(c);
    hipError_t e;
    const size_t sp = pitch64((size_t)sw), dp = pitch64((size_t)dw);
    Arena a{c};
    uint8_t* d_raw;
    const int st =
        upload_to_arena(a, img, (size_t)sw, sh, stride, dp * dh + 256, "remap staging", "upload raw image", &d_raw);
    if (st != ORB_OK) return st;
    uint8_t* d_out = a.take<uint8_t>(dp * dh);
    if ((e = launch_remap(1, &rect, d_raw, 1, sw, sh, 0, sp, d_out, 0, dp, c->stream)) != hipSuccess)
        return set_error("k_remap", e), ORB_ERR_HIP;
    if ((e = hipMemcpy2DAsync(dst, dst_stride, d_out, dp, dw, dh, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return set_error("download rectified image", e), ORB_ERR_HIP;
    return ORB_OK;
}

int orb_extract_rectified(orb_ctx* h, const orb_rectify* rect, const uint8_t* img, int sw, int sh, size_t stride,
                          orb_keypoint* kps, int cap, int* n, uint8_t* desc) {
    const char* const fn = "orb_extract_rectified";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const char* why = handles_fault(1, &rect, c)) return arg_error(fn, why);
    // (an empty image is judged first by its size: a NULL image of a positive size is orb_extract's empty image too)
    if (const char* why = remap_fault(1, sw, sh, rect->dw, rect->dh, 0, img ? stride : (size_t)-1, 0, 0, false))
        return arg_error(fn, why);
    CTX_GUARD(c);
    // _image.empty(), before or after the remap: outputs untouched (ORBextractor.cc:1046-1047)
    if (!img || sw == 0 || sh == 0 || rect->dw == 0 || rect->dh == 0) return ORB_OK;
    if (!n) return arg_error(fn, "n NULL");
    // the single-frame chain with the raw upload and k_remap in place of the gray upload; its image is the rectified
    // one, of the maps' size
    return extract_host(c, HostImage{img, sw, sh, stride, -1, rect}, kps, cap, n, desc);
}

}  // extern "C"
