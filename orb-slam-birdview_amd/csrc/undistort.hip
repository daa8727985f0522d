// Frame::UndistortKeyPoints and Frame::ComputeImageBounds (Frame.cc:571-660) with the fisheye model: the host twin
// (the definition, undistort.h), k_undistort_fisheye, and the creators that turn an extraction's output slots into
// resident frames (orb_frame) without staging the keypoints through the host.
#include <climits>
#include <cmath>
#include <limits>
#include <new>

#include "rgbd.h"
#include "undistort.h"

namespace orbgpu {

// The guard band.  The device's tan is not the host's; the kernel computes every result from scale and
// from scale * (1 -+ g), and a point whose three results differ in either coordinate is recomputed on the host.  The
// results are monotone in scale (every step is a correctly rounded monotone operation), so a point whose three results
// agree has the host's result as long as the host's scale lies within the band.  g is 16 times a bound of 8 ulps
// (2^-53 each) on |device tan - host tan|: above OpenCL's 5 ulps for tan plus glibc's 1, and 8 times the largest
// difference tools/tan_ulp_probe.hip measured on gfx950 (1 ulp over 3 x 2^24 arguments in [1e-8, 2]).
constexpr double kUndistortGuard = 0x1p-46;

constexpr int kUndistortThreads = 256;

// A point to recompute: its record's index in the output array and its raw position (the output may overwrite the
// input); the host sends the same record back with the host twin's result (bit patterns) in x, y.
struct UndistortRedo {
    int idx;
    uint32_t x, y;
};
static_assert(sizeof(UndistortRedo) == 12, "the redo list's record");
static_assert(sizeof(orb_keypoint) == 28, "k_undistort_fisheye copies 7 dwords");

void undistort_point_host(const Distortion& D, float x, float y, uint32_t& ox, uint32_t& oy) {
    const UndistortTheta t = undistort_theta(D, x, y);
    undistort_project(D, t, t.iterate ? std::tan(t.th) / t.th_d : 1.0, ox, oy);
}

// One lane per keypoint, frame blockIdx.y of a batch laid out as orb_extract_batch_device's outputs (frame f's records
// in slot f * in_step, at kp_cap records per slot, its count in counts[f * in_step]; counts == NULL: one frame of
// n_single).  The record is read as 7 dwords and written to out's slot f with x, y replaced; with in_step 1 out may be
// kps (a lane reads its record before it writes it and touches no other).
// Slots past a frame's count are not touched.  f64 throughout: the kernel is launch-bound (a few thousand lanes).
__global__ __launch_bounds__(kUndistortThreads) void k_undistort_fisheye(Distortion D, double g, const orb_keypoint* kps,
                                                                        const int* counts, int n_single, int kp_cap,
                                                                        int in_step, orb_keypoint* out, int* redo_count,
                                                                        UndistortRedo* redo) {
    const int f = blockIdx.y;
    const size_t slot = (size_t)f * (size_t)in_step;
    int n = counts ? counts[slot] : n_single;
    if (n > kp_cap) n = kp_cap;   // (the host refuses such a count once it has read it)
    const int i = blockIdx.x * kUndistortThreads + threadIdx.x;
    if (i >= n) return;
    const size_t r = (size_t)f * (size_t)kp_cap + (size_t)i;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(kps + slot * (size_t)kp_cap + (size_t)i);
    uint32_t w[7];
#pragma unroll
    for (int k = 0; k < 7; k++) w[k] = src[k];
    if (!D.identity) {
        const uint32_t rx = w[0], ry = w[1];
        const UndistortTheta t = undistort_theta(D, __uint_as_float(rx), __uint_as_float(ry));
        double scale = 1.0;
        if (t.iterate) scale = tan(t.th) / t.th_d;
        undistort_project(D, t, scale, w[0], w[1]);
        if (t.iterate) {
            uint32_t lx, ly, hx, hy;
            undistort_project(D, t, scale * (1.0 - g), lx, ly);
            undistort_project(D, t, scale * (1.0 + g), hx, hy);
            if (lx != w[0] || hx != w[0] || ly != w[1] || hy != w[1]) {
                const int at = atomicAdd(redo_count, 1);   // < nframes * kp_cap: a point appends once
                redo[at] = UndistortRedo{(int)r, rx, ry};
            }
        }
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + r);
#pragma unroll
    for (int k = 0; k < 7; k++) dst[k] = w[k];
}

// The host twin's results into their records (idx < total: checked by the host before the upload)
__global__ __launch_bounds__(kUndistortThreads) void k_undistort_patch(const UndistortRedo* __restrict__ redo, int n,
                                                                      orb_keypoint* out) {
    const int i = blockIdx.x * kUndistortThreads + threadIdx.x;
    if (i >= n) return;
    const UndistortRedo p = redo[i];
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + p.idx);
    dst[0] = p.x;
    dst[1] = p.y;
}

const char* distortion_fault(const orb_distortion* d) {
    if (!d) return "dist NULL";
    if (!std::isfinite(d->fx) || !std::isfinite(d->fy) || d->fx == 0.0f || d->fy == 0.0f)
        return "fx or fy zero or not finite";
    if (!std::isfinite(d->cx) || !std::isfinite(d->cy)) return "cx or cy not finite";
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(d->k[k])) return "a distortion coefficient is not finite";
    return nullptr;
}

// orb_frame_create's grid checks
const char* grid_fault(float min_x, float min_y, float inv_w, float inv_h) {
    if (!std::isfinite(inv_w) || !std::isfinite(inv_h) || inv_w <= 0 || inv_h <= 0)
        return "inverse cell size not finite or not positive";
    if (!std::isfinite(min_x) || !std::isfinite(min_y)) return "grid origin not finite";
    return nullptr;
}

const char* batch_fault(int nframes, int kp_cap) {
    if (nframes < 0) return "nframes < 0";
    if (nframes > 0 && kp_cap < 1) return "kp_cap < 1";
    if (nframes > 65535) return "more than 65,535 frames";
    if ((long long)nframes * (long long)kp_cap > (long long)INT_MAX) return "nframes * kp_cap above INT_MAX";
    return nullptr;
}

namespace {

double guard_of(const Ctx* c) { return c->undistort_guard > 0.0 ? c->undistort_guard : kUndistortGuard; }

// The counter cleared and the kernel queued (nframes >= 1, kp_cap >= 1)
hipError_t launch_undistort(const Distortion& D, double g, const orb_keypoint* d_in, const int* d_counts, int n_single,
                            int nframes, int kp_cap, int in_step, orb_keypoint* d_out, int* d_cnt,
                            UndistortRedo* d_list, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_cnt, 0, 4, stream);
    if (e != hipSuccess) return e;
    const int width = d_counts ? kp_cap : n_single;
    if (width <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_undistort_fisheye, dim3((width + kUndistortThreads - 1) / kUndistortThreads, nframes),
                       dim3(kUndistortThreads), 0, stream, D, g, d_in, d_counts, n_single, kp_cap, in_step, d_out, d_cnt,
                       d_list);
    return hipGetLastError();
}

// list (downloaded, the stream synchronised): every record recomputed by the host twin, sent back and scattered into
// d_out on the stream.  list stays alive until the caller has synchronised.
int patch_redone(const char* fn, Ctx* c, const Distortion& D, std::vector<UndistortRedo>& list, size_t total,
                 UndistortRedo* d_list, orb_keypoint* d_out) {
    if (list.empty()) return ORB_OK;
    for (UndistortRedo& p : list) {
        if (p.idx < 0 || (size_t)p.idx >= total)
            return set_error((std::string(fn) + ": redo list out of range").c_str(), hipSuccess), ORB_ERR_INTERNAL;
        float x, y;
        std::memcpy(&x, &p.x, 4);
        std::memcpy(&y, &p.y, 4);
        undistort_point_host(D, x, y, p.x, p.y);
    }
    hipError_t e = hipMemcpyAsync(d_list, list.data(), list.size() * sizeof(UndistortRedo), hipMemcpyHostToDevice,
                                  c->stream);
    if (e != hipSuccess) return set_error("undistort patch upload", e), ORB_ERR_HIP;
    const int n = (int)list.size();
    hipLaunchKernelGGL(k_undistort_patch, dim3((n + kUndistortThreads - 1) / kUndistortThreads), dim3(kUndistortThreads),
                       0, c->stream, d_list, n, d_out);
    if ((e = hipGetLastError()) != hipSuccess) return set_error("k_undistort_patch", e), ORB_ERR_HIP;
    return ORB_OK;
}

// Undistort a batch already on the device into d_out (which may be d_in); synchronised on return.
int undistort_device(const char* fn, Ctx* c, const Distortion& D, int nframes, const orb_keypoint* d_in,
                     const int* d_counts, int n_single, int kp_cap, orb_keypoint* d_out, int* d_cnt,
                     UndistortRedo* d_list, int* n_redone) {
    hipError_t e;
    int cnt = 0;
    if ((e = launch_undistort(D, guard_of(c), d_in, d_counts, n_single, nframes, kp_cap, 1, d_out, d_cnt, d_list,
                              c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return set_error(fn, e), ORB_ERR_HIP;
    const size_t total = (size_t)nframes * (size_t)kp_cap;
    if (cnt < 0 || (size_t)cnt > total)
        return set_error((std::string(fn) + ": redo count out of range").c_str(), hipSuccess), ORB_ERR_INTERNAL;
    if (cnt > 0) {
        std::vector<UndistortRedo> list((size_t)cnt);
        if ((e = hipMemcpyAsync(list.data(), d_list, list.size() * sizeof(UndistortRedo), hipMemcpyDeviceToHost,
                                c->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->stream)) != hipSuccess)
            return set_error(fn, e), ORB_ERR_HIP;
        const int st = patch_redone(fn, c, D, list, total, d_list, d_out);
        e = hipStreamSynchronize(c->stream);   // (list is read by the upload until here)
        if (st != ORB_OK) return st;
        if (e != hipSuccess) return set_error(fn, e), ORB_ERR_HIP;
    }
    if (n_redone) *n_redone = cnt;
    return ORB_OK;
}

}  // namespace

// orb_frame_create_from_extract (d_counts NULL, one frame of n_single keypoints, d_uright optional),
// orb_frames_create_from_batch, orb_frames_create_from_batch_rgbd (step kRgbd: the depth launch runs on the patched
// undistorted records, before any grid) and orb_frames_create_from_batch_stereo (step kStereo: frame f is slot 2 f of
// the batch, slot 2 f + 1 its right image; the search runs on the raw records in the same place).  The stream is
// synchronised three times at the most: after the undistort launch (the counts and the number of points to recompute),
// after the keypoints and the redo list have come to the host, and after the copies into the handles and the grid
// launches.
int frames_from_extract(const char* fn, Ctx* c, const orb_distortion* dist, int nframes, const uint8_t* d_desc,
                        const orb_keypoint* d_raw, const int* d_counts, int n_single, int kp_cap, const float* d_uright,
                        float min_x, float min_y, float inv_w, float inv_h, orb_frame** out, const DepthStep* step) {
    const bool batch = d_counts != nullptr;
    const bool stereo = step && step->kind == DepthStep::kStereo;
    const int slots = step ? step->slots() : 1;   // batch slots per frame
    const ProjGrid grid{min_x, min_y, inv_w, inv_h};
    CTX_GUARD(c);
    const Distortion D = widen(*dist);
    const size_t total = (size_t)nframes * (size_t)kp_cap;
    hipError_t e = hipSuccess;
    std::vector<orb_frame*> F((size_t)nframes, nullptr);
    std::vector<int> counts((size_t)nframes, n_single);
    std::vector<int> slot_counts;   // stereo: the counts of all 2 * nframes slots
    std::vector<UndistortRedo> list;
    auto fail = [&](const char* what, int st) {
        set_error(what, e);
        (void)hipStreamSynchronize(c->stream);   // queued copies write into the handles' memory
        for (orb_frame* f : F) orb_frame_destroy(f);
        return st;
    };
    // the arena: the undistorted records, the redo counter and list, every frame's k_frame_grid working space, a step's
    // mvuRight / mvDepth, and the stereo search's working space and match counts
    const size_t stereo_ints = stereo ? stereo_scratch_ints(c->geom, nframes, kp_cap) : 0;
    Arena a{c};
    if ((e = a.reserve(Arena::align(total * sizeof(orb_keypoint)) + Arena::align(total * sizeof(UndistortRedo)) +
                       Arena::align(2 * total * 4 + 256 * (size_t)nframes) + (step ? 2 * Arena::align(total * 4) : 0) +
                       (stereo ? Arena::align(stereo_ints * 4) + Arena::align((size_t)nframes * 4) : 0) + 2048)) !=
        hipSuccess)
        return fail("scratch", ORB_ERR_NOMEM);
    orb_keypoint* d_un = a.take<orb_keypoint>(total);
    int* d_cnt = a.take<int>(1);
    UndistortRedo* d_list = a.take<UndistortRedo>(total);
    // mvuRight / mvDepth of the batch, frame f's at f * kp_cap: the step's output (the caller's arrays or working
    // space), or without a step the caller's mvuRight of one frame
    float* const d_step_ur = !step ? nullptr : step->d_uright ? step->d_uright : a.take<float>(total);
    float* const d_step_depth = !step ? nullptr : step->d_depth ? step->d_depth : a.take<float>(total);
    const float* const d_ur_all = step ? d_step_ur : d_uright;
    int *d_stereo_work = nullptr, *d_stereo_matched = nullptr;
    if (stereo) {
        d_stereo_work = a.take<int>(stereo_ints);
        d_stereo_matched = a.take<int>((size_t)nframes);
        slot_counts.assign((size_t)nframes * 2, 0);
    }
    int* const counts_down = stereo ? slot_counts.data() : counts.data();
    int cnt = 0;
    if ((e = launch_undistort(D, guard_of(c), d_raw, d_counts, n_single, nframes, kp_cap, slots, d_un, d_cnt, d_list,
                              c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (batch && (e = hipMemcpyAsync(counts_down, d_counts, (size_t)nframes * slots * 4, hipMemcpyDeviceToHost,
                                      c->stream)) != hipSuccess))
        return fail("k_undistort_fisheye", ORB_ERR_HIP);
    // the handles; the single form knows its count before the first synchronisation, so its keypoints come down with
    // the counter
    auto make_frames = [&]() -> int {
        for (int f = 0; f < nframes; f++) {
            const int n = counts[f];
            if (n < 0 || n > kp_cap) {
                e = hipSuccess;
                return fail((std::string(fn) + ": a frame's count is negative or above kp_cap").c_str(), ORB_ERR_CAPACITY);
            }
            if (const char* what = frame_alloc(c, n, d_ur_all != nullptr, grid, F[f], e)) return fail(what, ORB_ERR_NOMEM);
            if (n > 0 && (e = hipMemcpyAsync(F[f]->kps.data(), d_un + (size_t)f * kp_cap, (size_t)n * sizeof(orb_keypoint),
                                             hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
                return fail("orb_frame keypoints to the host", ORB_ERR_HIP);
        }
        return ORB_OK;
    };
    int st;
    if (!batch && (st = make_frames()) != ORB_OK) return st;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail("undistort synchronise", ORB_ERR_HIP);
    if (cnt < 0 || (size_t)cnt > total) {
        e = hipSuccess;
        return fail((std::string(fn) + ": redo count out of range").c_str(), ORB_ERR_INTERNAL);
    }
    for (int f = 0; stereo && f < nframes; f++) {
        counts[f] = slot_counts[2 * f];
        // (the search sorts the right keypoints into kp_cap slots: a right count above them is refused as a left one is)
        if (slot_counts[2 * f + 1] < 0 || slot_counts[2 * f + 1] > kp_cap) counts[f] = -1;
    }
    if (batch && (st = make_frames()) != ORB_OK) return st;
    if (cnt > 0) {
        list.resize((size_t)cnt);
        if ((e = hipMemcpyAsync(list.data(), d_list, list.size() * sizeof(UndistortRedo), hipMemcpyDeviceToHost,
                                c->stream)) != hipSuccess)
            return fail("undistort redo list", ORB_ERR_HIP);
    }
    if ((batch || cnt > 0) && (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return fail("undistort synchronise", ORB_ERR_HIP);
    // the patch, in the device records and in the handles' host copies, before any grid is built
    if ((st = patch_redone(fn, c, D, list, total, d_list, d_un)) != ORB_OK) {
        (void)hipStreamSynchronize(c->stream);
        for (orb_frame* f : F) orb_frame_destroy(f);
        return st;
    }
    for (const UndistortRedo& p : list) {
        const int f = p.idx / kp_cap, i = p.idx % kp_cap;
        if (i < counts[f]) {
            std::memcpy(&F[f]->kps[i].x, &p.x, 4);
            std::memcpy(&F[f]->kps[i].y, &p.y, 4);
        }
    }
    // ComputeStereoFromRGBD on the final undistorted records (the patch is queued before it on the stream)
    if (step && !stereo && (e = launch_rgbd_depth(step->map, step->mbf, nframes, d_raw, d_un, d_counts, kp_cap, d_step_ur,
                                                  d_step_depth, nullptr, c->stream)) != hipSuccess)
        return fail("k_rgbd_depth", ORB_ERR_HIP);
    // ComputeStereoMatches on the raw records of the slot pairs, over the images and pyramids of the context's last batch
    if (stereo) {
        const StereoSide SL{c->last_frames, c->last_frame_pitch, c->last_row_stride, c->d_pyr.get(), 0, 2, d_raw, d_desc,
                            d_counts, kp_cap};
        StereoSide SR = SL;
        SR.frame0 = 1;
        if (c->prof_on) Ctx::marker(c, ORB_K_STEREO, 1, c->stream);
        e = launch_stereo(c->d_geom.get(), c->geom, SL, SR, nframes, step->mb, step->mbf, d_step_ur, d_step_depth,
                          d_stereo_work, kp_cap, d_stereo_matched, c->stream);
        if (c->prof_on) Ctx::marker(c, ORB_K_STEREO, 0, c->stream);
        if (e != hipSuccess) return fail("stereo kernels", ORB_ERR_HIP);
    }
    for (int f = 0; f < nframes; f++) {
        orb_frame* H = F[f];
        const size_t nn = (size_t)H->n;
        int* d_work = a.take<int>(2 * nn);
        if (nn > 0 &&
            ((e = hipMemcpyAsync(H->d_base.get(), d_desc + (size_t)f * slots * kp_cap * 32, nn * 32, hipMemcpyDeviceToDevice,
                                 c->stream)) != hipSuccess ||
             (e = hipMemcpyAsync(const_cast<orb_keypoint*>(H->d_kps), d_un + (size_t)f * kp_cap,
                                 nn * sizeof(orb_keypoint), hipMemcpyDeviceToDevice, c->stream)) != hipSuccess ||
             (d_ur_all && (e = hipMemcpyAsync(const_cast<float*>(H->d_ur), d_ur_all + (size_t)f * kp_cap, nn * 4,
                                              hipMemcpyDeviceToDevice, c->stream)) != hipSuccess)))
            return fail("orb_frame copy", ORB_ERR_HIP);
        if ((e = launch_frame_grid(H->d_kps, H->n, grid, const_cast<int*>(H->d_coff), const_cast<int*>(H->d_cidx), d_work,
                                   c->stream)) != hipSuccess)
            return fail("k_frame_grid", ORB_ERR_HIP);
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail("orb_frame synchronise", ORB_ERR_HIP);
    for (int f = 0; f < nframes; f++) {
        frame_octaves(F[f]);
        out[f] = F[f];
    }
    return ORB_OK;
}

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_undistort_points_host(const orb_distortion* dist, int n, const float* xy, float* xy_un) {
    const char* const fn = "orb_undistort_points_host";
    if (const char* why = distortion_fault(dist)) return arg_error(fn, why);
    if (n < 0) return arg_error(fn, "n < 0");
    if (n > 0 && (!xy || !xy_un)) return arg_error(fn, "NULL arrays with n > 0");
    const Distortion D = widen(*dist);
    if (D.identity) {
        if (n > 0 && xy_un != xy) std::memmove(xy_un, xy, (size_t)n * 8);
        return ORB_OK;
    }
    for (size_t i = 0; i < (size_t)n; i++) {
        uint32_t ox, oy;
        undistort_point_host(D, xy[2 * i], xy[2 * i + 1], ox, oy);
        std::memcpy(xy_un + 2 * i, &ox, 4);
        std::memcpy(xy_un + 2 * i + 1, &oy, 4);
    }
    return ORB_OK;
}

int orb_image_bounds(const orb_distortion* dist, int w, int h, float* min_x, float* max_x, float* min_y, float* max_y) {
    const char* const fn = "orb_image_bounds";
    if (const char* why = distortion_fault(dist)) return arg_error(fn, why);
    if (w < 0 || h < 0) return arg_error(fn, "negative image size");
    if (!min_x || !max_x || !min_y || !max_y) return arg_error(fn, "NULL output");
    if (dist->k[0] == 0.0f) {   // Frame.cc:653-659
        *min_x = 0.0f;
        *max_x = (float)w;
        *min_y = 0.0f;
        *max_y = (float)h;
        return ORB_OK;
    }
    const Distortion D = widen(*dist);
    const float corner[4][2] = {{0.0f, 0.0f}, {(float)w, 0.0f}, {0.0f, (float)h}, {(float)w, (float)h}};
    // Frame.cc:627-645: the maxima start at numeric_limits<float>::min(), the smallest positive normal float
    float mnx = std::numeric_limits<float>::max(), mxx = std::numeric_limits<float>::min(),
          mny = std::numeric_limits<float>::max(), mxy = std::numeric_limits<float>::min();
    for (int i = 0; i < 4; i++) {
        uint32_t bx, by;
        undistort_point_host(D, corner[i][0], corner[i][1], bx, by);
        float x, y;
        std::memcpy(&x, &bx, 4);
        std::memcpy(&y, &by, 4);
        if (x < mnx) mnx = x;
        if (x > mxx) mxx = x;
        if (y < mny) mny = y;
        if (y > mxy) mxy = y;
    }
    *min_x = mnx;
    *max_x = mxx;
    *min_y = mny;
    *max_y = mxy;
    return ORB_OK;
}

int orb_debug_undistort_guard(orb_ctx* h, double g) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    if (!(g >= 0.0) || !(g < 1.0)) return arg_error("orb_debug_undistort_guard", "g outside [0, 1)");
    c->undistort_guard = g;
    return ORB_OK;
}

int orb_undistort_keypoints(orb_ctx* h, const orb_distortion* dist, int n, const orb_keypoint* kps, orb_keypoint* kps_un,
                            int* n_redone) {
    const char* const fn = "orb_undistort_keypoints";
    if (const char* why = distortion_fault(dist)) return arg_error(fn, why);
    if (n < 0) return arg_error(fn, "n < 0");
    if (n > 0 && (!kps || !kps_un)) return arg_error(fn, "NULL arrays with n > 0");
    for (int i = 0; i < n; i++)
        if (!std::isfinite(kps[i].x) || !std::isfinite(kps[i].y)) return arg_error(fn, "keypoint position not finite");
    if (n == 0) {
        if (n_redone) *n_redone = 0;
        return ORB_OK;
    }
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    const size_t nn = (size_t)n;
    Arena a{c};
    hipError_t e = a.reserve(2 * Arena::align(nn * sizeof(orb_keypoint)) + Arena::align(nn * sizeof(UndistortRedo)) + 1024);
    if (e != hipSuccess) return set_error("scratch", e), ORB_ERR_NOMEM;
    orb_keypoint* d_in = a.take<orb_keypoint>(nn);
    orb_keypoint* d_out = a.take<orb_keypoint>(nn);
    int* d_cnt = a.take<int>(1);
    UndistortRedo* d_list = a.take<UndistortRedo>(nn);
    if ((e = hipMemcpyAsync(d_in, kps, nn * sizeof(orb_keypoint), hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return set_error(fn, e), ORB_ERR_HIP;
    int cnt = 0;
    const int st = undistort_device(fn, c, widen(*dist), 1, d_in, nullptr, n, n, d_out, d_cnt, d_list, &cnt);
    if (st != ORB_OK) return st;
    if ((e = hipMemcpyAsync(kps_un, d_out, nn * sizeof(orb_keypoint), hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return set_error(fn, e), ORB_ERR_HIP;
    if (n_redone) *n_redone = cnt;
    return ORB_OK;
}

int orb_undistort_keypoints_device(orb_ctx* h, const orb_distortion* dist, int nframes, const orb_keypoint* d_kps,
                                   const int* d_counts, int kp_cap, orb_keypoint* d_kps_un, int* n_redone) {
    const char* const fn = "orb_undistort_keypoints_device";
    if (const char* why = distortion_fault(dist)) return arg_error(fn, why);
    if (const char* why = batch_fault(nframes, kp_cap)) return arg_error(fn, why);
    if (nframes > 0 && (!d_kps || !d_counts || !d_kps_un)) return arg_error(fn, "NULL arrays with nframes > 0");
    if (nframes == 0) {
        if (n_redone) *n_redone = 0;
        return ORB_OK;
    }
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    const size_t total = (size_t)nframes * (size_t)kp_cap;
    Arena a{c};
    const hipError_t e = a.reserve(Arena::align(total * sizeof(UndistortRedo)) + 1024);
    if (e != hipSuccess) return set_error("scratch", e), ORB_ERR_NOMEM;
    int* d_cnt = a.take<int>(1);
    UndistortRedo* d_list = a.take<UndistortRedo>(total);
    return undistort_device(fn, c, widen(*dist), nframes, d_kps, d_counts, 0, kp_cap, d_kps_un, d_cnt, d_list, n_redone);
}

int orb_frame_create_from_extract(orb_ctx* h, const orb_distortion* dist, int n, const uint8_t* d_desc,
                                  const orb_keypoint* d_kps_raw, const float* d_uright, float min_x, float min_y,
                                  float inv_w, float inv_h, orb_frame** out) {
    const char* const fn = "orb_frame_create_from_extract";
    if (!out) return arg_error(fn, "out NULL");
    if (const char* why = distortion_fault(dist)) return arg_error(fn, why);
    if (n < 0) return arg_error(fn, "n < 0");
    if (n > 0 && (!d_desc || !d_kps_raw)) return arg_error(fn, "NULL arrays with n > 0");
    if (const char* why = grid_fault(min_x, min_y, inv_w, inv_h)) return arg_error(fn, why);
    // n == 0 is an empty frame, as for orb_frame_create: a handle all the same
    orb_frame* F = nullptr;
    const int st = frames_from_extract(fn, reinterpret_cast<Ctx*>(h), dist, 1, d_desc, d_kps_raw, nullptr, n,
                                       std::max(n, 1), d_uright, min_x, min_y, inv_w, inv_h, &F);
    if (st == ORB_OK) *out = F;
    return st;
}

int orb_frames_create_from_batch(orb_ctx* h, const orb_distortion* dist, int nframes, const uint8_t* d_desc,
                                 const orb_keypoint* d_kps_raw, const int* d_counts, int kp_cap, float min_x, float min_y,
                                 float inv_w, float inv_h, orb_frame** out) {
    const char* const fn = "orb_frames_create_from_batch";
    if (const char* why = distortion_fault(dist)) return arg_error(fn, why);
    if (const char* why = batch_fault(nframes, kp_cap)) return arg_error(fn, why);
    if (nframes > 0 && (!d_desc || !d_kps_raw || !d_counts || !out)) return arg_error(fn, "NULL arrays with nframes > 0");
    if (const char* why = grid_fault(min_x, min_y, inv_w, inv_h)) return arg_error(fn, why);
    if (nframes == 0) return ORB_OK;
    std::vector<orb_frame*> F((size_t)nframes, nullptr);
    const int st = frames_from_extract(fn, reinterpret_cast<Ctx*>(h), dist, nframes, d_desc, d_kps_raw, d_counts, 0, kp_cap,
                                       nullptr, min_x, min_y, inv_w, inv_h, F.data());
    if (st == ORB_OK)
        for (int f = 0; f < nframes; f++) out[f] = F[f];
    return st;
}

}  // extern "C"
