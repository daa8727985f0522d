// Device-resident map points (orb_points, include/orbgpu.h) and their projection: Frame::isInFrustum and the
// projection loop of Fuse on the GPU, one lane per point (point_project.h has the arithmetic).  The fused searches
// over the projected queries are matcher.hip's (orb_search_local_points, orb_fuse_search_points).
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "point_project.h"

namespace orbgpu {

// Item i: slot ids[i] through its camera.  The record goes to rec[i]; the query a grid search takes for it to pq[i]
// and the slot's descriptor to qdesc + 32 i, so k_projection_topk / k_projection_best read what a staged call would
// have uploaded.  ids were validated by the host (0 <= id < capacity), item_cam is the host's own.
__global__ __launch_bounds__(256) void k_project_points(int mode, const PointCam* __restrict__ cams,
                                                        const int* __restrict__ item_cam,
                                                        const int* __restrict__ ids, int n,
                                                        const PointGeo* __restrict__ geo,
                                                        const uint8_t* __restrict__ pdesc,
                                                        orb_point_proj* __restrict__ rec,
                                                        orb_proj_query* __restrict__ pq,
                                                        uint8_t* __restrict__ qdesc) {
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    const PointCam& C = cams[item_cam ? item_cam[i] : 0];
    const float4* gp = reinterpret_cast<const float4*>(geo + id);
    const float4 a = gp[0], b = gp[1];
    const PointGeo g{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    orb_proj_query Q;
    const orb_point_proj o = project_point(mode, C, g, Q);
    if (rec) rec[i] = o;
    if (pq) pq[i] = Q;
    if (qdesc) {
        const uint4* dp = reinterpret_cast<const uint4*>(pdesc + (long long)id * 32);
        uint4* qp = reinterpret_cast<uint4*>(qdesc + (long long)i * 32);
        qp[0] = dp[0];
        qp[1] = dp[1];
    }
}

hipError_t launch_project_points(int mode, const PointCam* d_cams, const int* d_item_cam, const int* d_ids, int n,
                                 const PointGeo* d_geo, const uint8_t* d_pdesc, orb_point_proj* rec,
                                 orb_proj_query* d_pq, uint8_t* d_qdesc, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_project_points, dim3((n + 255) / 256), dim3(256), 0, stream, mode, d_cams, d_item_cam, d_ids, n,
                       d_geo, d_pdesc, rec, d_pq, d_qdesc);
    return hipGetLastError();
}

// T[k] = the smallest positive finite float r with ceilf(logf(r) / lsf) > k, by bisection over the bit patterns of
// the positive floats (they ascend with the value) with the host's own logf; +inf when no finite r reaches level
// k + 1.  The bisection rests on ceilf(logf(r) / lsf) not decreasing in r (tests/test_frustum_pin.py checks the
// thresholds against the direct form around every threshold and on a million ratios).
void level_thresholds(float lsf, int nlevels, float* T) {
    auto from_bits = [](uint32_t b) {
        float f;
        std::memcpy(&f, &b, 4);
        return f;
    };
    for (int k = 0; k < ORBGPU_MAX_LEVELS; k++) T[k] = INFINITY;
    for (int k = 0; k + 1 < nlevels; k++) {
        auto above = [&](uint32_t b) { return std::ceil(std::log(from_bits(b)) / lsf) > (float)k; };
        uint32_t lo = 1, hi = 0x7f7fffffu;   // the smallest denormal, FLT_MAX
        if (!above(hi)) continue;
        if (above(lo)) {
            T[k] = from_bits(lo);
            continue;
        }
        while (hi - lo > 1) {   // above(lo) is false, above(hi) true
            const uint32_t mid = lo + (hi - lo) / 2;
            (above(mid) ? hi : lo) = mid;
        }
        T[k] = from_bits(hi);
    }
}

const char* camera_fault(const orb_camera* K) {
    if (!K) return "camera NULL";
    if (K->nlevels < 1 || K->nlevels > ORBGPU_MAX_LEVELS) return "nlevels outside [1, ORBGPU_MAX_LEVELS]";
    if (!(K->log_scale_factor > 0) || !std::isfinite(K->log_scale_factor)) return "log_scale_factor not finite or <= 0";
    const float* f = K->Rcw;   // Rcw, tcw, Ow, fx .. mbf, min_x .. max_y: 24 consecutive floats
    static_assert(offsetof(orb_camera, nlevels) == 24 * sizeof(float), "orb_camera's leading floats");
    for (int i = 0; i < 24; i++)
        if (!std::isfinite(f[i])) return "camera field not finite";
    for (int l = 0; l < K->nlevels; l++)
        if (!std::isfinite(K->scale_factors[l])) return "camera field not finite";
    return nullptr;
}

const char* frustum_scalars_fault(float view_cos_limit, float th) {
    if (!std::isfinite(th) || th < 0) return "th not finite or negative";
    if (!std::isfinite(view_cos_limit)) return "view_cos_limit not finite";
    return nullptr;
}

// The kernel indexes the slots by ids: every one is checked here
const char* point_ids_fault(const orb_points* P, int n, const int* ids) {
    if (!P) return "NULL points handle";
    if (n < 0) return "n < 0";
    if (n > 0 && !ids) return "ids NULL with n > 0";
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= P->cap) return "id outside [0, capacity)";
    return nullptr;
}

PointCam point_cam(Ctx* c, const orb_camera& cam, float view_cos_limit, float th) {
    PointCam P{};
    P.cam = cam;
    for (int l = cam.nlevels; l < ORBGPU_MAX_LEVELS; l++) P.cam.scale_factors[l] = 0.0f;   // (never read)
    P.th = th;
    P.view_cos_limit = view_cos_limit;
    if (c)
        for (const Ctx::LevelThresholds& L : c->level_thr)
            if (std::memcmp(&L.lsf, &cam.log_scale_factor, 4) == 0 && L.nlevels == cam.nlevels) {
                std::memcpy(P.T, L.T, sizeof P.T);
                return P;
            }
    level_thresholds(cam.log_scale_factor, cam.nlevels, P.T);
    if (c) {
        Ctx::LevelThresholds L{cam.log_scale_factor, cam.nlevels, {}};
        std::memcpy(L.T, P.T, sizeof P.T);
        if (c->level_thr.size() >= 16) c->level_thr.clear();   // (a SLAM run has one or two settings)
        c->level_thr.push_back(L);
    }
    return P;
}

namespace {

// The device layout of cap slots: [geo | desc]
size_t points_desc_off(size_t cap) { return Arena::align(cap * sizeof(PointGeo)); }
size_t points_bytes(size_t cap) { return points_desc_off(cap) + cap * 32; }

// P adopts base (allocated for cap slots, or for one where cap is 0); base leaves with P's previous allocation
void points_bind(orb_points* P, DevBuf<uint8_t>& base, int cap) {
    P->d_base.swap(base);
    P->cap = cap;
    P->d_geo = reinterpret_cast<const PointGeo*>(P->d_base.get());
    P->d_desc = P->d_base.get() + points_desc_off((size_t)cap);
}

}  // namespace
}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_points_create(orb_ctx* h, int capacity, orb_points** out) {
    const char* const fn = "orb_points_create";
    if (!out) return arg_error(fn, "out NULL");
    if (capacity < 0) return arg_error(fn, "capacity < 0");
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    orb_points* P = new (std::nothrow) orb_points();
    if (!P) return set_error("orb_points", hipSuccess), ORB_ERR_NOMEM;
    P->device = c->device;
    DevBuf<uint8_t> base;
    const hipError_t e = base.ensure(points_bytes((size_t)std::max(capacity, 1)));
    if (e != hipSuccess) {
        delete P;
        return set_error("orb_points allocation", e), ORB_ERR_NOMEM;
    }
    points_bind(P, base, capacity);
    *out = P;
    return ORB_OK;
}

int orb_points_write(orb_points* P, int first, int n, const float* pos, const float* normal, const float* min_dist,
                     const float* max_dist, const uint8_t* desc) {
    const char* const fn = "orb_points_write";
    if (!P) return arg_error(fn, "NULL handle");
    if (first < 0 || n < 0) return arg_error(fn, "negative first or n");
    if ((long long)first + (long long)n > (long long)INT_MAX) return arg_error(fn, "slot range beyond INT_MAX");
    if (n > 0 && (!pos || !normal || !min_dist || !max_dist || !desc)) return arg_error(fn, "NULL arrays with n > 0");
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(pos[3 * (size_t)i + k]) || !std::isfinite(normal[3 * (size_t)i + k]))
                return arg_error(fn, "position or normal not finite");
        if (!std::isfinite(min_dist[i]) || !std::isfinite(max_dist[i])) return arg_error(fn, "distance not finite");
    }
    if (n == 0) return ORB_OK;
    hipError_t e = hipSetDevice(P->device);
    if (e != hipSuccess) return set_error("hipSetDevice", e), ORB_ERR_HIP;
    const int need = first + n;
    if (need > P->cap) {
        // at least doubled; hipFree waits for the device, so queued work that reads the old allocation ends first
        const long long want = std::max<long long>(need, 2LL * P->cap);
        const int cap = (int)std::min<long long>(want, INT_MAX);
        DevBuf<uint8_t> base;
        if ((e = base.ensure(points_bytes((size_t)cap))) != hipSuccess)
            return set_error("orb_points growth", e), ORB_ERR_NOMEM;
        if (P->cap > 0 &&
            ((e = hipMemcpy(base.get(), P->d_geo, (size_t)P->cap * sizeof(PointGeo), hipMemcpyDeviceToDevice)) !=
                 hipSuccess ||
             (e = hipMemcpy(base.get() + points_desc_off((size_t)cap), P->d_desc, (size_t)P->cap * 32,
                            hipMemcpyDeviceToDevice)) != hipSuccess))
            return set_error("orb_points growth copy", e), ORB_ERR_HIP;
        points_bind(P, base, cap);
    }
    std::vector<PointGeo> geo;
    try {
        geo.resize((size_t)n);
    } catch (const std::bad_alloc&) {
        return set_error("orb_points_write staging", hipSuccess), ORB_ERR_NOMEM;
    }
    for (size_t i = 0; i < (size_t)n; i++)
        geo[i] = PointGeo{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], normal[3 * i], normal[3 * i + 1],
                          normal[3 * i + 2], min_dist[i], max_dist[i]};
    // plain hipMemcpy from pageable memory: both have completed on the device when they return
    if ((e = hipMemcpy(P->d_base.get() + (size_t)first * sizeof(PointGeo), geo.data(), (size_t)n * sizeof(PointGeo),
                       hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(P->d_base.get() + points_desc_off((size_t)P->cap) + (size_t)first * 32, desc, (size_t)n * 32,
                       hipMemcpyHostToDevice)) != hipSuccess)
        return set_error("orb_points_write", e), ORB_ERR_HIP;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return set_error("orb_points_write synchronise", e), ORB_ERR_HIP;
    return ORB_OK;
}

int orb_points_capacity(const orb_points* P) { return P ? P->cap : 0; }

void orb_points_destroy(orb_points* P) {
    if (!P) return;
    // the allocation is freed even where the device cannot be made current: hipFree takes a pointer, not the
    // current device
    (void)hipSetDevice(P->device);
    delete P;
}

int orb_project_points(orb_ctx* h, const orb_points* P, int mode, const orb_camera* camera, float view_cos_limit,
                       float th, int n, const int* ids, orb_point_proj* proj_out) {
    const char* const fn = "orb_project_points";
    if (mode != ORB_FRUSTUM_FRAME && mode != ORB_FRUSTUM_FUSE) return arg_error(fn, "unknown mode");
    if (const char* why = camera_fault(camera)) return arg_error(fn, why);
    if (const char* why = frustum_scalars_fault(view_cos_limit, th)) return arg_error(fn, why);
    if (const char* why = point_ids_fault(P, n, ids)) return arg_error(fn, why);
    if (n > 0 && !proj_out) return arg_error(fn, "proj_out NULL");
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    if (P->device != c->device) return arg_error(fn, "the points live on another device");
    CTX_GUARD(c);
    if (n == 0) return ORB_OK;
    // [camera | ids] go up in one DMA; the kernel stores the records straight into the pinned mirror
    Stage st{c};
    const size_t o_cam = st.add(sizeof(PointCam)), o_ids = st.add((size_t)n * 4), o_in_end = st.off,
                 o_rec = st.add((size_t)n * sizeof(orb_point_proj));
    const int r = st.alloc();
    if (r != ORB_OK) return r;
    *st.hi<PointCam>(o_cam) = point_cam(c, *camera, view_cos_limit, th);
    st.put(o_ids, ids, (size_t)n * 4);
    hipError_t e;
    if ((e = st.up(0, o_in_end)) != hipSuccess) return set_error("upload", e), ORB_ERR_HIP;
    if ((e = launch_project_points(mode, st.di<PointCam>(o_cam), nullptr, st.di<int>(o_ids), n, P->d_geo, P->d_desc,
                                   st.h<orb_point_proj>(o_rec), nullptr, nullptr, c->stream)) != hipSuccess)
        return set_error("k_project_points", e), ORB_ERR_HIP;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return set_error("orb_project_points", e), ORB_ERR_HIP;
    std::memcpy(proj_out, st.h<orb_point_proj>(o_rec), (size_t)n * sizeof(orb_point_proj));
    return ORB_OK;
}

int orb_project_points_host(int mode, const orb_camera* camera, float view_cos_limit, float th, int n, const float* pos,
                            const float* normal, const float* min_dist, const float* max_dist,
                            orb_point_proj* proj_out) {
    const char* const fn = "orb_project_points_host";
    if (mode != ORB_FRUSTUM_FRAME && mode != ORB_FRUSTUM_FUSE) return arg_error(fn, "unknown mode");
    if (const char* why = camera_fault(camera)) return arg_error(fn, why);
    if (const char* why = frustum_scalars_fault(view_cos_limit, th)) return arg_error(fn, why);
    if (n < 0) return arg_error(fn, "n < 0");
    if (n > 0 && (!pos || !normal || !min_dist || !max_dist || !proj_out)) return arg_error(fn, "NULL arrays with n > 0");
    const PointCam C = point_cam(nullptr, *camera, view_cos_limit, th);
    for (size_t i = 0; i < (size_t)n; i++) {
        orb_proj_query Q;
        proj_out[i] = project_point(mode, C,
                                    PointGeo{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], normal[3 * i],
                                             normal[3 * i + 1], normal[3 * i + 2], min_dist[i], max_dist[i]},
                                    Q);
    }
    return ORB_OK;
}

}  // extern "C"
