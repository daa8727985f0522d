// Device-resident Frame / KeyFrame handles (orb_frame, include/orbgpu.h): the train side of the grid searches,
// uploaded once, and Frame::AssignFeaturesToGrid (Frame.cc:378-413) on the GPU.
#include <cmath>
#include <cstring>
#include <new>

#include "frame_cell.h"
#include "undistort.h"

namespace orbgpu {

constexpr int kGridThreads = 1024;
constexpr int kGridWaves = kGridThreads / 64;
constexpr int kGridCellsPerThread = kFrameGridCells / kGridThreads;   // 3
constexpr int kGridBlockSeg = 1024;   // a cell with more keypoints than this is ordered by the whole workgroup
static_assert(kGridCellsPerThread * kGridThreads == kFrameGridCells, "k_frame_grid's scan");

// The Frame grid CSR of n keypoints, one workgroup:
//   1. each keypoint's cell (frame_cell) goes to cell_of[i] and counts into an LDS counter of its cell;
//   2. an exclusive scan of the 3,072 counters gives cell_off (LDS and global);
//   3. every keypoint is scattered to the next free slot of its cell in tmp (LDS atomic cursor: any order);
//   4. each cell's segment is written to cell_idx in ascending keypoint index, the order of the reference's push_back
//      loop.  The indices of a segment are distinct, so an index's place is the number of smaller ones in its segment:
//      a wave per cell, a lane per index, counting over the segment (most segments hold a few indices).  A segment
//      above kGridBlockSeg is not counted (quadratic) but rebuilt: the workgroup walks all keypoints in index order
//      and compacts those of that cell, 1,024 per step, so all keypoints in one cell cost n / 1,024 steps.
// cell_of and tmp are n ints each of working space.  Indices are ints throughout (n above 65,535 is fine).
__global__ __launch_bounds__(kGridThreads) void k_frame_grid(const orb_keypoint* __restrict__ kps, int n, ProjGrid g,
                                                            int* __restrict__ cell_off, int* __restrict__ cell_idx,
                                                            int* cell_of, int* tmp) {
    __shared__ int s_cnt[kFrameGridCells];       // counts, then scatter cursors
    __shared__ int s_off[kFrameGridCells + 1];
    __shared__ int s_wave[kGridWaves];
    __shared__ unsigned short s_long[kFrameGridCells];   // the cells above kGridBlockSeg, in any order
    __shared__ int s_nlong;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = tid; c < kFrameGridCells; c += kGridThreads) s_cnt[c] = 0;
    if (tid == 0) s_nlong = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kGridThreads) {
        const int c = frame_cell(kps[i].x, kps[i].y, g.min_x, g.min_y, g.inv_w, g.inv_h);
        cell_of[i] = c;
        if (c >= 0) atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan: a thread's 3 consecutive cells, the wave's threads, the waves
    int cnt[kGridCellsPerThread], mine = 0;
#pragma unroll
    for (int k = 0; k < kGridCellsPerThread; k++) {
        cnt[k] = s_cnt[tid * kGridCellsPerThread + k];
        mine += cnt[k];
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = incl - mine;
    for (int w = 0; w < wave; w++) before += s_wave[w];
#pragma unroll
    for (int k = 0; k < kGridCellsPerThread; k++) {
        const int c = tid * kGridCellsPerThread + k;
        s_off[c] = before;
        s_cnt[c] = before;   // (each thread rewrites the counters it read itself)
        cell_off[c] = before;
        before += cnt[k];
        if (cnt[k] > kGridBlockSeg) s_long[atomicAdd(&s_nlong, 1)] = (unsigned short)c;
    }
    if (tid == kGridThreads - 1) {
        s_off[kFrameGridCells] = before;
        cell_off[kFrameGridCells] = before;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kGridThreads) {
        const int c = cell_of[i];
        if (c >= 0) tmp[atomicAdd(&s_cnt[c], 1)] = i;   // slot < cell_off[c + 1] <= n
    }
    __syncthreads();   // (tmp and cell_of are read below by other threads of this workgroup)
    for (int c = wave; c < kFrameGridCells; c += kGridWaves) {
        const int s0 = s_off[c], len = s_off[c + 1] - s0;
        if (len > kGridBlockSeg) continue;
        for (int e = lane; e < len; e += 64) {
            const int v = tmp[s0 + e];
            int rank = 0;
            for (int j = 0; j < len; j++) rank += tmp[s0 + j] < v;
            cell_idx[s0 + rank] = v;   // rank < len
        }
    }
    for (int k = 0, nlong = s_nlong; k < nlong; k++) {   // (the same cells for every thread)
        const int c = s_long[k], s0 = s_off[c];
        int done = 0;
        for (int i0 = 0; i0 < n; i0 += kGridThreads) {
            const int i = i0 + tid;
            const bool in = i < n && cell_of[i] == c;
            const unsigned long long m = __ballot(in);
            __syncthreads();   // the previous step's s_wave has been read
            if (lane == 0) s_wave[wave] = __popcll(m);
            __syncthreads();
            int pos = done + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
            for (int w = 0; w < kGridWaves; w++) {
                if (w < wave) pos += s_wave[w];
                total += s_wave[w];
            }
            if (in) cell_idx[s0 + pos] = i;   // pos < len: the cell holds len keypoints
            done += total;
        }
    }
}

hipError_t launch_frame_grid(const orb_keypoint* d_kps, int n, const ProjGrid& g, int* d_cell_off, int* d_cell_idx,
                             int* d_work, hipStream_t stream) {
    if (n <= 0) return hipMemsetAsync(d_cell_off, 0, (size_t)(kFrameGridCells + 1) * 4, stream);
    hipLaunchKernelGGL(k_frame_grid, dim3(1), dim3(kGridThreads), 0, stream, d_kps, n, g, d_cell_off, d_cell_idx, d_work,
                       d_work + n);
    return hipGetLastError();
}

const char* frame_alloc(Ctx* c, int n, bool has_ur, const ProjGrid& g, orb_frame*& out, hipError_t& e) {
    out = nullptr;
    orb_frame* F = new (std::nothrow) orb_frame();
    if (!F) return "orb_frame";
    F->device = c->device;
    F->n = n;
    F->has_ur = has_ur;
    F->min_x = g.min_x;
    F->min_y = g.min_y;
    F->inv_w = g.inv_w;
    F->inv_h = g.inv_h;
    // [desc | kps | uright | cell_off | cell_idx], each region 256-byte aligned
    const size_t nn = (size_t)n;
    const size_t o_kps = Arena::align(nn * 32), o_ur = Arena::align(o_kps + nn * sizeof(orb_keypoint)),
                 o_coff = Arena::align(o_ur + nn * 4), o_cidx = Arena::align(o_coff + (size_t)(kFrameGridCells + 1) * 4);
    if ((e = F->d_base.ensure(Arena::align(o_cidx + nn * 4))) != hipSuccess) {
        delete F;
        return "orb_frame allocation";
    }
    const uint8_t* const base = F->d_base.get();
    F->d_desc = base;
    F->d_kps = reinterpret_cast<const orb_keypoint*>(base + o_kps);
    F->d_ur = has_ur ? reinterpret_cast<const float*>(base + o_ur) : nullptr;
    F->d_coff = reinterpret_cast<const int*>(base + o_coff);
    F->d_cidx = reinterpret_cast<const int*>(base + o_cidx);
    try {
        F->kps.resize(nn);
    } catch (const std::bad_alloc&) {
        delete F;
        return "orb_frame host keypoints";
    }
    out = F;
    return nullptr;
}

void frame_octaves(orb_frame* F) {   // (orb_fuse_search_points checks them against its camera's nlevels per call)
    for (int i = 0; i < F->n; i++) {
        const int o = F->kps[i].octave;
        F->oct_min = i ? std::min(F->oct_min, o) : o;
        F->oct_max = i ? std::max(F->oct_max, o) : o;
    }
}

namespace {

// Both creators: src_kind says where desc / kps / uright live.  The keypoints come to the host copy (from the host
// array, or once from the device), the grid is built on the context's stream, and the call returns synchronised.
int frame_create(const char* fn, Ctx* c, int n, const uint8_t* desc, const orb_keypoint* kps, const float* uright,
                 float min_x, float min_y, float inv_w, float inv_h, hipMemcpyKind src_kind, orb_frame** out) {
    if (!out) return arg_error(fn, "out NULL");
    if (n < 0) return arg_error(fn, "n < 0");
    if (n > 0 && (!desc || !kps)) return arg_error(fn, "NULL arrays with n > 0");
    if (const char* why = grid_fault(min_x, min_y, inv_w, inv_h)) return arg_error(fn, why);
    if (src_kind == hipMemcpyHostToDevice)
        for (int i = 0; i < n; i++)
            if (!std::isfinite(kps[i].x) || !std::isfinite(kps[i].y))
                return arg_error(fn, "keypoint position not finite");
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return set_error("hipSetDevice", e), ORB_ERR_HIP;
    const ProjGrid g{min_x, min_y, inv_w, inv_h};
    orb_frame* F = nullptr;
    auto fail = [&](const char* what, int st) {
        set_error(what, e);
        // copies already queued write into F's allocation and F's host keypoints: they end before either is released
        (void)hipStreamSynchronize(c->stream);
        delete F;
        return st;
    };
    if (const char* what = frame_alloc(c, n, uright != nullptr, g, F, e)) return fail(what, ORB_ERR_NOMEM);
    // k_frame_grid's working space is the context's scratch arena, free again once this call has synchronised.
    // reserve() frees and reallocates the arena when it has to grow (hipFree waits for the device, so queued work that
    // reads the old arena ends first): like every user of the arena this relies on no caller keeping a pointer into it
    // across calls.  That holds for an extraction context too (the device form): the extraction's buffers and the
    // batch outputs are allocations of their own, and only the matcher calls and this one take from the arena.
    const size_t nn = (size_t)n;
    Arena a{c};
    if ((e = a.reserve(Arena::align(2 * nn * 4) + 512)) != hipSuccess) return fail("scratch", ORB_ERR_NOMEM);
    int* d_work = a.take<int>(2 * nn);
    if (n > 0) {
        if (src_kind == hipMemcpyHostToDevice) std::memcpy(F->kps.data(), kps, nn * sizeof(orb_keypoint));
        if ((e = hipMemcpyAsync(const_cast<uint8_t*>(F->d_desc), desc, nn * 32, src_kind, c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(const_cast<orb_keypoint*>(F->d_kps), kps, nn * sizeof(orb_keypoint), src_kind, c->stream)) !=
                hipSuccess ||
            (uright && (e = hipMemcpyAsync(const_cast<float*>(F->d_ur), uright, nn * 4, src_kind, c->stream)) != hipSuccess))
            return fail("orb_frame copy", ORB_ERR_HIP);
        if (src_kind == hipMemcpyDeviceToDevice &&
            (e = hipMemcpyAsync(F->kps.data(), kps, nn * sizeof(orb_keypoint), hipMemcpyDeviceToHost, c->stream)) !=
                hipSuccess)
            return fail("orb_frame keypoints to the host", ORB_ERR_HIP);
    }
    if ((e = launch_frame_grid(F->d_kps, n, g, const_cast<int*>(F->d_coff), const_cast<int*>(F->d_cidx), d_work,
                               c->stream)) != hipSuccess)
        return fail("k_frame_grid", ORB_ERR_HIP);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail("orb_frame synchronise", ORB_ERR_HIP);
    frame_octaves(F);
    *out = F;
    return ORB_OK;
}

}  // namespace
}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_frame_create(orb_ctx* h, int n, const uint8_t* desc, const orb_keypoint* kps_un, const float* uright,
                     float min_x, float min_y, float inv_w, float inv_h, orb_frame** out) {
    return frame_create("orb_frame_create", reinterpret_cast<Ctx*>(h), n, desc, kps_un, uright, min_x, min_y, inv_w,
                        inv_h, hipMemcpyHostToDevice, out);
}

int orb_frame_create_device(orb_ctx* h, int n, const uint8_t* d_desc, const orb_keypoint* d_kps, const float* d_uright,
                            float min_x, float min_y, float inv_w, float inv_h, orb_frame** out) {
    return frame_create("orb_frame_create_device", reinterpret_cast<Ctx*>(h), n, d_desc, d_kps, d_uright, min_x, min_y,
                        inv_w, inv_h, hipMemcpyDeviceToDevice, out);
}

void orb_frame_destroy(orb_frame* F) {
    if (!F) return;
    // the allocation is freed even where the device cannot be made current: hipFree takes a pointer, not the
    // current device
    (void)hipSetDevice(F->device);
    delete F;
}

int orb_frame_count(const orb_frame* F) { return F ? F->n : 0; }

int orb_frame_grid_read(const orb_frame* F, int* cell_off, int* cell_idx, int cap, int* nslots) {
    const char* const fn = "orb_frame_grid_read";
    if (!F || !cell_off || cap < 0 || (cap > 0 && !cell_idx)) return arg_error(fn, "bad arguments");
    hipError_t e = hipSetDevice(F->device);
    if (e != hipSuccess) return set_error("hipSetDevice", e), ORB_ERR_HIP;
    if ((e = hipMemcpy(cell_off, F->d_coff, (size_t)(kFrameGridCells + 1) * 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return set_error("orb_frame_grid_read", e), ORB_ERR_HIP;
    const int ns = cell_off[kFrameGridCells];
    if (nslots) *nslots = ns;
    if (ns > cap) return set_error("orb_frame_grid_read: cell_idx too small", hipSuccess), ORB_ERR_CAPACITY;
    if (ns > 0 && (e = hipMemcpy(cell_idx, F->d_cidx, (size_t)ns * 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return set_error("orb_frame_grid_read", e), ORB_ERR_HIP;
    return ORB_OK;
}

}  // extern "C"
