// The projection of one map point through one camera (orb_point_proj, include/orbgpu.h): Frame::isInFrustum
// (Frame.cc:436-492) with the search radius of ORBmatcher.cc:63-69, and the projection loop of Fuse(KeyFrame*,
// vector<MapPoint*>, th) (ORBmatcher.cc:852-890), with MapPoint::PredictScale (MapPoint.cc:385-417).  One function for
// the kernel (points.hip) and the host restatement (orb_project_points_host): both translation units are built
// -ffp-contract=off, so the fmaf below are the only fused operations, and they are the reference build's
// (tools/frustum_flags_probe.cpp); float division, double division and double sqrt are correctly rounded on both sides.
#pragma once
#include <cmath>

#include "orbgpu_ctx.h"

namespace orbgpu {

// A slot's geometry on the device (32 B: two 16-byte loads)
struct PointGeo {
    float px, py, pz, nx, ny, nz, min_dist, max_dist;
};
static_assert(sizeof(PointGeo) == 32, "k_project_points' record layout");

// What a launch reads per camera: the camera, the level thresholds of its (log_scale_factor, nlevels) and the two
// scalars of the call.  T[k], k = 0 .. nlevels - 2, is the smallest positive float r with ceilf(logf(r) / lsf) > k
// by the host's logf (+inf: no finite r); level = #{k : ratio >= T[k]}.
struct PointCam {
    orb_camera cam;
    float T[ORBGPU_MAX_LEVELS];
    float th, view_cos_limit;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define ORBGPU_PP_FINITE(x) (__builtin_isfinite(x))
#else
#define ORBGPU_PP_FINITE(x) (std::isfinite(x))
#endif

// cv::Mat Rcw * P + tcw for one row: OpenCV's GEMMSingleMul accumulates float products in double, left to right, adds
// the (double) t and rounds once (the model of tests/cpp/cv_api/opencv2/core/core.hpp)
__host__ __device__ inline float pp_row(const float* R, float p0, float p1, float p2, float t) {
    const double s = ((double)R[0] * (double)p0 + (double)R[1] * (double)p1) + (double)R[2] * (double)p2;
    return (float)(s + (double)t);
}

__host__ __device__ inline int pp_level(const PointCam& C, float max_dist, float dist) {
    const float ratio = max_dist / dist;
    if (!ORBGPU_PP_FINITE(ratio)) return 0;
    int level = 0;
    for (int k = 0; k < C.cam.nlevels - 1; k++) level += ratio >= C.T[k];
    return level;
}

// The record of point g; Q receives the query the grid searches take for a visible point, and a window no train can
// lie in (r = 0, far outside every grid) otherwise.
__host__ __device__ inline orb_point_proj project_point(int mode, const PointCam& C, const PointGeo& g,
                                                       orb_proj_query& Q) {
    const orb_camera& K = C.cam;
    orb_point_proj o{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1, ORB_POINT_VISIBLE};
    Q = orb_proj_query{-1.0e6f, -1.0e6f, 0.0f, -1, -1, 0.0f, 0.0f, 0.0f, 1};
    const float PcX = pp_row(K.Rcw + 0, g.px, g.py, g.pz, K.tcw[0]);
    const float PcY = pp_row(K.Rcw + 3, g.px, g.py, g.pz, K.tcw[1]);
    const float PcZ = pp_row(K.Rcw + 6, g.px, g.py, g.pz, K.tcw[2]);
    if (PcZ < 0.0f) return o.verdict = ORB_POINT_DEPTH, o;
    const float invz = 1.0f / PcZ;
    o.invz = invz;
    const bool fuse = mode == ORB_FRUSTUM_FUSE;
    if (fuse) {
        const float x = PcX * invz, y = PcY * invz;
        o.u = fmaf(K.fx, x, K.cx);
        o.v = fmaf(K.fy, y, K.cy);
        if (!(o.u >= K.min_x && o.u < K.max_x && o.v >= K.min_y && o.v < K.max_y)) return o.verdict = ORB_POINT_BOUNDS, o;
        o.ur = fmaf(-K.mbf, invz, o.u);
    } else {
        o.u = fmaf(K.fx * PcX, invz, K.cx);
        o.v = fmaf(K.fy * PcY, invz, K.cy);
        if (o.u < K.min_x || o.u > K.max_x) return o.verdict = ORB_POINT_BOUNDS, o;
        if (o.v < K.min_y || o.v > K.max_y) return o.verdict = ORB_POINT_BOUNDS, o;
    }
    const float POx = g.px - K.Ow[0], POy = g.py - K.Ow[1], POz = g.pz - K.Ow[2];
    const double n2 = ((double)POx * (double)POx + (double)POy * (double)POy) + (double)POz * (double)POz;
    const float dist = (float)sqrt(n2);
    o.dist = dist;
    if (dist < 0.8f * g.min_dist || dist > 1.2f * g.max_dist) return o.verdict = ORB_POINT_DISTANCE, o;
    const double dot = ((double)POx * (double)g.nx + (double)POy * (double)g.ny) + (double)POz * (double)g.nz;
    float r0;
    if (fuse) {
        if (dot < 0.5 * (double)dist) return o.verdict = ORB_POINT_ANGLE, o;
        r0 = C.th;
    } else {
        const float view_cos = (float)(dot / (double)dist);
        o.view_cos = view_cos;
        if (view_cos < C.view_cos_limit) return o.verdict = ORB_POINT_ANGLE, o;
        o.ur = fmaf(-K.mbf, invz, o.u);
        r0 = (double)view_cos > 0.998 ? 2.5f : 4.0f;
        if (C.th != 1.0f) r0 *= C.th;
    }
    o.level = pp_level(C, g.max_dist, dist);
    o.r = r0 * K.scale_factors[o.level];
    if (!ORBGPU_PP_FINITE(o.u) || !ORBGPU_PP_FINITE(o.v) || !ORBGPU_PP_FINITE(o.ur) || !ORBGPU_PP_FINITE(o.r))
        return o.verdict = ORB_POINT_NOT_FINITE, o;
    Q = orb_proj_query{o.u, o.v, o.r, o.level - 1, o.level, o.ur, fuse ? 0.0f : o.r, 0.0f, 1};
    return o;
}

}  // namespace orbgpu

// Map points resident on the device (the object behind orb_points*): one allocation [geo | desc], cap slots each.
struct orb_points {
    int device = 0;
    int cap = 0;
    orbgpu::DevBuf<uint8_t> d_base;
    const orbgpu::PointGeo* d_geo = nullptr;
    const uint8_t* d_desc = nullptr;
};

namespace orbgpu {

// The thresholds of (log_scale_factor, nlevels), from the host's logf (points.hip; cached per context)
void level_thresholds(float log_scale_factor, int nlevels, float* T);
// What is wrong with a camera / the scalars / the handle and ids of a projection call, or NULL
const char* camera_fault(const orb_camera* cam);
const char* frustum_scalars_fault(float view_cos_limit, float th);
const char* point_ids_fault(const orb_points* points, int n, const int* ids);
// The device's record of a (validated) camera; ctx (or NULL) caches the thresholds
PointCam point_cam(Ctx* ctx, const orb_camera& cam, float view_cos_limit, float th);

// k_project_points (points.hip): item i projects slot ids[i] through cams[item_cam ? item_cam[i] : 0].  rec (n
// records; may be host-coherent memory), pq and qdesc (n queries and their gathered descriptors, the inputs of
// k_projection_topk / k_projection_best) may each be NULL.
hipError_t launch_project_points(int mode, const PointCam* d_cams, const int* d_item_cam, const int* d_ids, int n,
                                 const PointGeo* d_geo, const uint8_t* d_pdesc, orb_point_proj* rec,
                                 orb_proj_query* d_pq, uint8_t* d_qdesc, hipStream_t stream);

}  // namespace orbgpu
