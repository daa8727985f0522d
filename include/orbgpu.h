/*
 * orbgpu.h — C-ABI of the MI355X-native ORB front-end (gfx950 HIP kernels).
 *
 * Drop-in boundary for the ORB front-end of donglinb/ORB-SLAM-BIRDVIEW.  Each entry point names the
 * reference interface it replaces; the C++ mirror classes ORB_SLAM2::ORBextractor / ORBmatcher
 * (orb-slam-birdview_amd/csrc/host/) and the Python binding (orbgpu/) are thin layers over it.
 *
 *  - Plain pointers and sizes only: no HIP, torch or OpenCV types in any signature.
 *  - Nothing throws across the ABI; every function returns an orb_status (0 = OK).
 *  - A context owns one HIP stream on one device; entry points call hipSetDevice on entry, so a
 *    context may be driven from any host thread (Frame.cc:124-127 spawns fresh threads per frame),
 *    but one context must not be used by two threads at once (same contract as the reference's
 *    one-extractor-per-thread, ORBextractor.h:85 mvImagePyramid is instance state).
 *  - There is no CPU fallback: if the HIP runtime or device is unavailable, orb_create fails.
 */
#ifndef ORBGPU_H
#define ORBGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBGPU_ABI_VERSION 2
#define ORBGPU_MAX_LEVELS 16

/* OpenCV arithmetic variant (orb_params.variant / orb_bird_params.variant, bit flags).  The reference
 * links whichever OpenCV 2.4.3-3.4 the build machine has (CMakeLists.txt:31-37) and calls its resize
 * (ORBextractor.cc:1120) and GaussianBlur (:1085-1086); those versions differ in the last bits, and the
 * octree sort (:684) breaks size ties by heap address.  0 is the pinned default (OpenCV 3.2 x86-64 SSE2
 * without IPP; ties by node creation sequence; BRIEF offsets contracted to FMA as GCC -march=native
 * builds them).  The bit values equal the oracle's ORACLE_* flags (oracle/orb_oracle.h). */
#define ORB_VARIANT_DEFAULT        0
#define ORB_VARIANT_TIE_REVERSE    1  /* :684 tie: a later-created node counts as the SMALLER pointer      */
#define ORB_VARIANT_RESIZE_GENERIC 2  /* resize vertical pass = generic FixedPtCast (b0*H0+b1*H1+2^21)>>22 */
#define ORB_VARIANT_BLUR_HALFUP    4  /* GaussianBlur column pass rounds half-up everywhere (no SSE2 body) */
#define ORB_VARIANT_NO_FMA         8  /* BRIEF sample offsets (:119-120) uncontracted (no -march=native FMA) */
#define ORB_VARIANT_MASK          15

typedef enum {
    ORB_OK = 0,
    ORB_ERR_ARG = -1,        /* bad argument / NULL pointer                                     */
    ORB_ERR_HIP = -2,        /* HIP runtime error (message via orb_last_error)                   */
    ORB_ERR_CAPACITY = -3,   /* caller buffer too small; *n receives the required count          */
    ORB_ERR_GEOMETRY = -4,   /* image too small for the pyramid (reference: division by zero UB), a side
                                above 4096 pixels (candidates pack 12-bit coordinates), or a level whose
                                octree node tables exceed one CU's LDS (N per level above 2,488: 2,496 nodes of
                                64 bytes; about nfeatures 11,450 at scale 1.2 / 8 levels, 2,488 at one level) */
    ORB_ERR_NOMEM = -5,      /* device allocation failed                                         */
    ORB_ERR_INTERNAL = -6    /* a kernel reported an overflow of an internal bound               */
} orb_status;

/* Bit-compatible with cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id;}
 * (28 bytes), so the OpenCV-side adapter can memcpy. */
typedef struct {
    float x, y, size, angle, response;
    int octave, class_id;
} orb_keypoint;

/* ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
 * replaces ORBextractor::ORBextractor, reference src/ORBextractor.cc:410-470 / include/ORBextractor.h:52-53 */
typedef struct {
    int nfeatures;
    float scaleFactor;
    int nlevels;
    int iniThFAST;
    int minThFAST;
    int device;       /* HIP device ordinal                                     */
    int max_width;    /* capacity hints (contexts grow on demand for host input) */
    int max_height;
    int max_batch;    /* frames per batched launch (device-resident path)       */
    int variant;      /* ORB_VARIANT_* bits (0 = pinned default); unknown bits: ORB_ERR_ARG */
} orb_params;

typedef struct orb_ctx orb_ctx;

int  orb_abi_version(void);
const char* orb_last_error(void);      /* thread-local message for the last failure */
int  orb_device_count(void);

orb_ctx* orb_create(const orb_params* p, int* status);
void     orb_destroy(orb_ctx* ctx);

/* GetLevels/GetScaleFactor(s)/GetInverseScaleFactors/GetScaleSigmaSquares/GetInverseScaleSigmaSquares
 * (include/ORBextractor.h:63-83) + mnFeaturesPerLevel (ORBextractor.cc:435-446) + umax (:454-469).
 * Any pointer may be NULL. Arrays hold nlevels entries (umax: 16). */
int orb_scale_tables(const orb_ctx* ctx, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                     int* n_per_level, int* umax16);

/* ORBextractor::operator()(InputArray image, InputArray mask, vector<KeyPoint>&, OutputArray)
 * — reference src/ORBextractor.cc:1043-1105.  Host gray image in (mask ignored, as in the reference,
 * include/ORBextractor.h:58); keypoints (level-0 coordinates, level-major order) and n x 32
 * descriptors out.  Empty image (w==0 || h==0 || img==NULL) returns ORB_OK leaving *n and the
 * outputs untouched (:1046-1047).  If *n would exceed cap, returns ORB_ERR_CAPACITY with *n set. */
int orb_extract(orb_ctx* ctx, const uint8_t* img, int w, int h, size_t stride,
                orb_keypoint* kps, int cap, int* n, uint8_t* desc);

/* public std::vector<cv::Mat> mvImagePyramid (include/ORBextractor.h:85), read by
 * Frame::ComputeStereoMatches (Frame.cc:669,759): host view of level `level` of the last
 * orb_extract, copied lazily device->host into context-owned memory (valid until the next call). */
int orb_get_level(orb_ctx* ctx, int level, const uint8_t** data, int* w, int* h, size_t* stride);

/* ---- device-resident batched path (bench, multi-camera streams). Asynchronous on the context
 * stream; call orb_sync before reading outputs. d_frames: nframes gray frames, frame f at
 * d_frames + f*frame_pitch, rows `row_stride` apart (w <= row_stride < 16 MiB).  Outputs: frame f's keypoints at
 * d_kps + f*kp_cap, descriptors at d_desc + f*kp_cap*32, count in d_counts[f].
 * kp_cap must be >= orb_batch_kp_cap(ctx, w, h). ---- */
int orb_batch_kp_cap(orb_ctx* ctx, int w, int h);
int orb_extract_batch_device(orb_ctx* ctx, const uint8_t* d_frames, int nframes, int w, int h,
                             size_t frame_pitch, size_t row_stride,
                             orb_keypoint* d_kps, uint8_t* d_desc, int* d_counts, int kp_cap);
int orb_sync(orb_ctx* ctx);

/* device memory helpers (so callers need no HIP headers) */
void* orb_device_alloc(orb_ctx* ctx, size_t bytes);
int   orb_device_free(orb_ctx* ctx, void* p);
int   orb_memcpy_h2d(orb_ctx* ctx, void* dst, const void* src, size_t bytes);
int   orb_memcpy_d2h(orb_ctx* ctx, void* dst, const void* src, size_t bytes);
int   orb_memset_device(orb_ctx* ctx, void* dst, int value, size_t bytes);

/* ---- per-kernel timing with HIP events on the context stream (bench roofline) ---- */
enum { ORB_K_RESIZE = 0, ORB_K_FAST = 1, ORB_K_OCTREE = 2, ORB_K_DESCRIBE = 3, ORB_K_HAMMING = 4,
       ORB_K_STEREO = 5, ORB_K_FLOW = 6 /* the small-batch dataflow launch: every stage in one kernel */,
       ORB_K_COUNT = 7 };
int orb_profile_enable(orb_ctx* ctx, int on);   /* clears accumulated times */
int orb_profile_read(orb_ctx* ctx, double* ms_total /*ORB_K_COUNT*/, int* launches /*ORB_K_COUNT*/);

/* ---- debug views of intermediate device buffers (parity tests pinpoint the failing stage) ---- */
/* FAST candidates of `level` for frame `frame` of the last batch, in vToDistributeKeys order
 * (ORBextractor.cc:820-825): 3 ints (x, y, score) each, coords relative to minBorder. */
int orb_debug_candidates(orb_ctx* ctx, int frame, int level, int* out, int cap);
/* Octree output of `level` (DistributeOctTree list order): 3 ints (x, y, score), level coords. */
int orb_debug_level_keypoints(orb_ctx* ctx, int frame, int level, int* out, int cap);
int orb_debug_level_image(orb_ctx* ctx, int frame, int level, uint8_t* out, int* w, int* h);
/* Phase timestamps of the last FAST launch (diagnostic; only with ORBGPU_FAST_STAMPS=1 in the
 * environment at orb_create): 8 s_memtime values per (frame, cell) item.  With ORBGPU_FLOW_STAMPS=1 instead,
 * the last dataflow launch's: 4 values per task in ticket order (100 MHz s_memrealtime when its ticket was
 * taken, when its wait ended, when it was done; then kind | level << 8 | frame << 16 | workgroup << 32).
 * Returns the count copied. */
int orb_debug_fast_stamps(orb_ctx* ctx, uint64_t* out, int cap);
/* The BRIEF rotation's sin/cos as the kernels compute them (glibc sinf/cosf restated, ORBextractor.cc:113)
 * for n host angles (radians, 0 <= x < 120): s[i] = sinf(x[i]), c[i] = cosf(x[i]).  Pin test only. */
int orb_debug_sincosf(orb_ctx* ctx, const float* x, int n, float* s, float* c);

/* =========================== Birdview stream (Frame.cc:318-342) ===========================
 * The reference runs OpenCV's cv::ORB (HARRIS_SCORE, not ORBextractor) plus cv::cornerSubPix on the
 * birdview image.  orb_bird mirrors cv::ORB::create(nfeatures, scaleFactor, nlevels, edgeThreshold,
 * firstLevel 0, WTA_K 2, HARRIS_SCORE, patchSize 31, fastThreshold) — Frame.cc:329 uses
 * ORB::create(2000): {2000, 1.2f, 8, 31, 20}.  One HIP stream per object; one host thread at a time. */
typedef struct {
    int nfeatures;
    float scaleFactor;
    int nlevels;
    int edgeThreshold;
    int fastThreshold;
    int device;
    int variant;      /* ORB_VARIANT_RESIZE_GENERIC | ORB_VARIANT_BLUR_HALFUP apply (cv::ORB's own pyramid
                         resize and descriptor blur, orb.cpp); other bits: ORB_ERR_ARG */
} orb_bird_params;

typedef struct orb_bird orb_bird;

orb_bird* orb_bird_create(const orb_bird_params* p, int* status);
void      orb_bird_destroy(orb_bird* b);

/* cv::ORB::detect(image, keypoints, mask) — Frame.cc:330 (OpenCV 3.2 ORB_Impl::detectAndCompute,
 * computeKeyPoints).  mask may be NULL (no mask).  Keypoints in level-0 coordinates, reference order.
 * Empty image: *n = 0.  cap too small: ORB_ERR_CAPACITY with *n set. */
int orb_bird_detect(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, const uint8_t* mask,
                    size_t mask_stride, orb_keypoint* kps, int cap, int* n);
/* cv::ORB::compute(image, keypoints, descriptors) — Frame.cc:342.  kps in/out: border-culled
 * (runByImageBorder, edgeThreshold) and level-sorted in place, *n updated; desc receives *n x 32. */
int orb_bird_compute(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, orb_keypoint* kps, int* n,
                     uint8_t* desc);
/* cv::cornerSubPix(image, pts (n x float2, in/out), Size(win_w, win_h), Size(-1,-1),
 * TermCriteria(EPS+MAX_ITER, max_iter, eps)) — Frame.cc:336-337.  Only Size(5,5) is built. */
int orb_corner_subpix(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, float* pts, int n, int win_w,
                      int win_h, int max_iter, double eps);
/* Frame.cc:320-342 fused: footprint-masked detect, cornerSubPix(5x5, 40, 0.001), compute — one upload,
 * one pyramid.  mask (birdviewMask) is not modified: the footprint is zeroed in the device copy. */
int orb_bird_extract(orb_bird* b, const uint8_t* img, int w, int h, size_t stride, const uint8_t* mask,
                     size_t mask_stride, orb_keypoint* kps, int cap, int* n, uint8_t* desc);
/* Same, image and mask already in device memory (bench / multi-stream callers). */
int orb_bird_extract_device(orb_bird* b, const uint8_t* d_img, int w, int h, size_t stride, const uint8_t* d_mask,
                            size_t mask_stride, orb_keypoint* kps, int cap, int* n, uint8_t* desc);
/* Frame.cc:320-342 for nframes birdview images of one size in one call: every stage before the keypoint
 * selection is one launch over all frames, the host selects frame by frame, and the selected keypoints go
 * through cornerSubPix / compute in groups behind the host.  0 <= nframes <= ORB_BIRD_MAX_BATCH.
 *   device form: frame f starts at d_imgs + f * frame_pitch (frame_pitch >= stride * h), its mask at
 *     d_masks + f * mask_frame_pitch; mask_frame_pitch 0: one mask shared by all frames (its pyramid is
 *     built once per call); d_masks NULL: no mask.
 *   host form: imgs[f] are host pointers; masks has nmasks entries: 0 (none), 1 (shared) or nframes.
 * Masks are the caller's birdviewMask and are not modified (footprint zeroed in the device copy).
 * Outputs are host memory: frame f's keypoints at kps + f * cap, descriptors at desc + f * cap * 32, count
 * in counts[f]; each frame's output is byte for byte what orb_bird_extract_device returns for that frame
 * and mask alone.  Slots past counts[f] are not written.
 * Errors: ORB_ERR_ARG (before any GPU work, outputs untouched) for nframes out of range, NULL counts,
 * NULL kps / desc with cap > 0, stride < w, mask_stride < w with a mask, a frame pitch below stride * h,
 * nmasks not in {0, 1, nframes}.  nframes 0: ORB_OK, nothing touched.  w <= 0 or h <= 0: every count 0,
 * ORB_OK.  ORB_ERR_CAPACITY when any counts[f] > cap: all counts are set, frames that fit are written in
 * full, frames that do not are left untouched.  ORB_ERR_GEOMETRY / ORB_ERR_NOMEM as in the single call.
 * Single and batch calls may alternate on one object at any sizes; the buffers of a size grow to the
 * largest batch seen at that size and are reused (a new size starts again from the batch it is called
 * with).  Device memory by the pyramid formulas: three pyramids (image, FAST score, blur) of about 3.0 MB
 * and a candidate slot of about 12 MB per 1280x720 frame, plus a mask pyramid per frame with per-frame
 * masks (one in all with a shared mask): about 24 MB per frame, about 1.5 GB at ORB_BIRD_MAX_BATCH.
 * orb_bird_debug_candidates / orb_bird_debug_level are unspecified after a batch call. */
#define ORB_BIRD_MAX_BATCH 64
int orb_bird_extract_batch_device(orb_bird* b, int nframes, const uint8_t* d_imgs, int w, int h, size_t stride,
                                  size_t frame_pitch, const uint8_t* d_masks, size_t mask_stride,
                                  size_t mask_frame_pitch, orb_keypoint* kps, uint8_t* desc, int cap, int* counts);
int orb_bird_extract_batch(orb_bird* b, int nframes, const uint8_t* const* imgs, int w, int h, size_t stride,
                           const uint8_t* const* masks, int nmasks, size_t mask_stride, orb_keypoint* kps,
                           uint8_t* desc, int cap, int* counts);
/* Frames per post-selection group of the batch calls (keypoint upload + angle / subpix / desc launches
 * that run while the host selects the next group).  group > 0 sets it (clamped to ORB_BIRD_MAX_BATCH);
 * returns the value in force.  Results do not depend on it. */
int orb_bird_batch_group(orb_bird* b, int group);
/* Frame.cc:320-327: zero the vehicle footprint (+15 px boundary) of a birdview mask in place (host). */
int orb_bird_footprint_mask(uint8_t* mask, int w, int h, size_t stride);
/* debug: last detect's level-l candidates after mask / border / NMS, raster order, level coordinates;
 * response = Harris response, class_id = FAST score.  Returns the count (or -count-1 if cap is too small). */
int orb_bird_debug_candidates(orb_bird* b, int level, orb_keypoint* out, int cap);
int orb_bird_debug_level(orb_bird* b, int level, uint8_t* out, int* w, int* h);

/* =========================== ORBmatcher =========================== */

/* static int ORBmatcher::DescriptorDistance(const cv::Mat&, const cv::Mat&)  ORBmatcher.cc:1647-1663
 * (host helper: a single pair is never worth a kernel launch). */
int orb_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Top-k smallest Hamming distances per query on the GPU (the inner loop of every ORBmatcher search).
 * Candidates of query i: cand_idx[cand_off[i] .. cand_off[i+1]) (CSR, in the reference's iteration
 * order), or all trains 0..nt-1 if cand_off == NULL.  A candidate t is skipped when
 * train_thr != NULL and train_thr[t] <= dist (covers vbMatched2 / vMatchedDistance / invalid
 * MapPoints).  Results sorted by (dist, candidate position): out_dist/out_idx[i*k + j], -1 padded;
 * out_nvalid[i] = number of candidates that passed the filter (tells whether the list is complete).
 * Host pointers, synchronous. */
int orb_hamming_topk(orb_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                     const int* cand_off, const int* cand_idx, const int* train_thr, int k,
                     int* out_dist, int* out_idx, int* out_nvalid);

/* Device-pointer variant of the all-pairs (cand_off == NULL, no filter) top-2: best distance,
 * its train index (first on ties) and second-best distance per query. Asynchronous. */
int orb_hamming_top2_device(orb_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                            int* d_best, int* d_best_idx, int* d_second);

/* Batched device form over the descriptor slots of an extraction batch (orb_extract_batch_device's
 * d_desc / d_counts / kp_cap): pair p matches the descriptors of frame q_frames[p] against those of
 * frame t_frames[p] (host arrays), all pairs in one launch, counts read on the device.  Outputs at
 * d_best / d_best_idx / d_second[p * kp_cap + i].  kp_cap <= 65535.  Asynchronous.  This is the
 * brute-force SearchByBoW inner loop of BASELINE config C4 (one vocabulary node holding everything). */
int orb_hamming_top2_frames_device(orb_ctx* ctx, const uint8_t* d_desc, const int* d_counts, int kp_cap, int npairs,
                                   const int* q_frames, const int* t_frames, int* d_best, int* d_best_idx,
                                   int* d_second);

/* Train slices one top-2 launch splits each pair into for these sizes (orb_hamming_top2_device passes
 * npairs = 1; the frames form passes kp_cap for both maxima).  1 = the MFMA kernel writes best / index /
 * second itself; more = per-slice partial results merged by a second kernel.  Host only (test / tuning). */
int orb_hamming_top2_slices(int npairs, int max_nq, int max_nt);

/* Operand width of the all-pairs top-2's matrix-core form: 4 = +-4 e2m1 fp4 (v_mfma_scale_f32_32x32x64_f8f6f4,
 * bound by the dense FP4 peak; the only form since round 5).  Host only (bench / tests). */
int orb_hamming_top2_mfma_bits(void);

/* DBoW2::FeatureVector (std::map<NodeId, vector<unsigned>>, FeatureVector.h:21) as CSR.  The three
 * FeatureVector matchers below return ORB_ERR_ARG (before any GPU work) for a CSR whose offsets do not start at
 * 0 or decrease, whose indices leave [0, n) of their side, or whose node ids do not ascend strictly. */
typedef struct {
    int nnodes;
    const uint32_t* node_ids;   /* ascending */
    const int* offsets;         /* nnodes + 1 */
    const int* indices;
} orb_featvec;

/* int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)
 * ORBmatcher.cc:159-288.  mp_kf[i]!=0 <=> KF feature i has a non-bad MapPoint; angles are
 * mvKeysUn (KF) / mvKeys (F) angles.  match_f[iF] = KF feature index whose MapPoint was assigned
 * to F feature iF, or -1.  *nmatches receives the return value of the reference function. */
int orb_search_by_bow_kf_f(orb_ctx* ctx, float nnratio, int check_ori,
                           int n_kf, const uint8_t* desc_kf, const float* angle_kf, const uint8_t* mp_kf,
                           orb_featvec fv_kf, int n_f, const uint8_t* desc_f, const float* angle_f,
                           orb_featvec fv_f, int* match_f, int* nmatches);

/* int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
 * ORBmatcher.cc:522-655.  match12[i1] = KF2 feature index whose MapPoint was assigned, or -1. */
int orb_search_by_bow_kf_kf(orb_ctx* ctx, float nnratio, int check_ori,
                            int n1, const uint8_t* desc1, const float* angle1, const uint8_t* mp1,
                            orb_featvec fv1, int n2, const uint8_t* desc2, const float* angle2,
                            const uint8_t* mp2, orb_featvec fv2, int* match12, int* nmatches);

/* The BoW searches over several keyframes in one call (one staging, one ranking launch, then each keyframe's
 * replay in the reference's order): the loops of Tracking::Relocalization (Tracking.cc:1931-1938,
 * SearchByBoW(pKF, mCurrentFrame, ...) per candidate keyframe) and LoopClosing::ComputeSim3 (LoopClosing.cc:252-265,
 * SearchByBoW(mpCurrentKF, pKF, ...) per loop candidate), whose iterations are independent.  Entry p's outputs are
 * exactly the single call's for the same inputs.
 *   orb_search_by_bow_kf_f_batch:  KF = kfs[p] (n, desc, angle, mp = its map-point flags, fv) against one Frame;
 *                                  match = match_f (n_f ints), *nmatches = the return value.
 *   orb_search_by_bow_kf_kf_batch: KF1 against KF2 = kf2s[p] (mp = KF2's map-point flags); match = match12 (n1 ints).
 * ORB_ERR_ARG for a malformed entry (nothing runs). */
typedef struct orb_bow_kf {
    int n;
    const uint8_t* desc;
    const float* angle;
    const uint8_t* mp;
    orb_featvec fv;
    int* match;
    int* nmatches;
} orb_bow_kf;
int orb_search_by_bow_kf_f_batch(orb_ctx* ctx, float nnratio, int check_ori, int n_f, const uint8_t* desc_f,
                                 const float* angle_f, orb_featvec fv_f, int nkf, const orb_bow_kf* kfs);
int orb_search_by_bow_kf_kf_batch(orb_ctx* ctx, float nnratio, int check_ori, int n1, const uint8_t* desc1,
                                  const float* angle1, const uint8_t* mp1, orb_featvec fv1, int nkf,
                                  const orb_bow_kf* kf2s);

/* int ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12,
 *     vector<pair<size_t,size_t>>&, const bool bOnlyStereo)   ORBmatcher.cc:657-823
 * Keypoints are mvKeysUn; has_mp[i] <=> GetMapPoint(i) != NULL; uright = mvuRight; F12 row-major
 * 3x3; (ex, ey) the epipole of KF1's centre in KF2 (:662-668, computed by the caller from poses);
 * scale2/sigma2_2 = pKF2->mvScaleFactors / mvLevelSigma2.  pairs_out: 2 ints per pair (ascending
 * idx1), *npairs = count (ORB_ERR_CAPACITY if > cap).  ORB_ERR_ARG for a malformed FeatureVector CSR (see
 * orb_featvec; the call stages at most offsets[nnodes] records per side). */
int orb_search_for_triangulation(orb_ctx* ctx, int check_ori, int only_stereo,
                                 int n1, const uint8_t* desc1, const orb_keypoint* kps1, const uint8_t* has_mp1,
                                 const float* uright1, orb_featvec fv1,
                                 int n2, const uint8_t* desc2, const orb_keypoint* kps2, const uint8_t* has_mp2,
                                 const float* uright2, orb_featvec fv2,
                                 const float* F12, float ex, float ey, const float* scale2, const float* sigma2_2,
                                 int nlevels2, int* pairs_out, int cap, int* npairs);

/* SearchForTriangulation of one keyframe (KF1) against several (KF2s) in one call: LocalMapping::CreateNewMapPoints
 * (LocalMapping.cc:247-278) calls SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, ..., false) once per
 * neighbour keyframe.  pairs[p] carries what the single call takes for KF2 = pair p (its outputs included);
 * the result for pair p is exactly orb_search_for_triangulation's for the same inputs, all pairs sharing one
 * staging, one launch and one synchronisation.  The reference loop adds map points to KF1 between neighbours
 * (:449), and SearchForTriangulation skips KF1 features that have one (:694-696); with check_ori = 0 (the
 * LocalMapping call) every query is decided independently, so a caller that drops, while it walks the pairs in
 * order, the matches of pair p whose idx1 received a map point from pairs < p gets the sequential result exactly.
 * ORB_ERR_ARG for a malformed pair (nothing runs); ORB_ERR_CAPACITY if any pair's list overflowed (every pair's
 * *npairs holds its full count, the lists are filled up to cap). */
typedef struct orb_tri_pair {
    int n2;
    const uint8_t* desc2;
    const orb_keypoint* kps2;
    const uint8_t* has_mp2;
    const float* uright2;
    orb_featvec fv2;
    const float* F12;            /* row-major 3x3 */
    float ex, ey;                /* KF1's centre projected in KF2 */
    const float* scale2;         /* pKF2->mvScaleFactors */
    const float* sigma2_2;       /* pKF2->mvLevelSigma2 */
    int nlevels2;                /* entries of scale2 / sigma2_2, in [1, ORBGPU_MAX_LEVELS]; every keypoint of kps2 has
                                    its octave in [0, nlevels2).  Otherwise the call (the single form and the batch
                                    alike) returns ORB_ERR_ARG and writes nothing for any pair */
    int* pairs_out;              /* 2 ints per pair */
    int cap;
    int* npairs;
} orb_tri_pair;
int orb_search_for_triangulation_batch(orb_ctx* ctx, int check_ori, int only_stereo,
                                       int n1, const uint8_t* desc1, const orb_keypoint* kps1, const uint8_t* has_mp1,
                                       const float* uright1, orb_featvec fv1, int npairs, const orb_tri_pair* pairs);

/* int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<Point2f>& vbPrevMatched,
 *     vector<int>& vnMatches12, int windowSize)  ORBmatcher.cc:405-520 (level0_only = 1), and
 * int ORBmatcher::BirdviewMatch(const Frame&, const Frame&, vector<int>&, int)  :1790-1899
 * (level0_only = 0).  Candidates per query = Frame::GetFeaturesInArea (CSR), computed by the caller
 * (orb_features_in_area restates it).  match12 out. */
int orb_window_match(orb_ctx* ctx, float nnratio, int check_ori, int level0_only,
                     int n1, const uint8_t* desc1, const orb_keypoint* kps1,
                     int n2, const uint8_t* desc2, const orb_keypoint* kps2,
                     const int* cand_off, const int* cand_idx, int* match12, int* nmatches);

/* The Frame grid as the reference holds it (Frame.h:211 mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS], filled by
 * Frame::AssignFeaturesToGrid, Frame.cc:378-413) flattened column-major: the keypoints of cell (ix, iy)
 * are cell_idx[cell_off[ix * 48 + iy] .. cell_off[ix * 48 + iy + 1]) in the cell vector's order; the cell
 * arithmetic of Frame::GetFeaturesInArea (:494-547) uses min_x / min_y and the inverse cell sizes.  The
 * birdview grid (GetFeaturesInAreaBirdview, :891-945) is the same with min_x = min_y = 0. */
typedef struct orb_frame_grid {
    float min_x, min_y;          /* mnMinX, mnMinY */
    float inv_w, inv_h;          /* mfGridElementWidthInv, mfGridElementHeightInv */
    const int* cell_off;         /* 64 * 48 + 1 */
    const int* cell_idx;         /* cell_off[64 * 48] entries */
} orb_frame_grid;

/* The window searches with the candidate lists computed on the GPU from F2's grid: the same matches
 * as orb_window_match with cand = GetFeaturesInArea(centre, window, octave1, octave1) per query.
 * centres: n1 (x, y) pairs (SearchForInitialization's vbPrevMatched, BirdviewMatch's vPrevMatched), or
 * NULL = each query's own keypoint position (BirdviewMatch(const Frame&, const Frame&, ...), :1803-1808).
 * level0_only: queries with octave > 0 are skipped (:420-423, :1683-1685).  match12 out. */
int orb_window_match_grid(orb_ctx* ctx, float nnratio, int check_ori, int level0_only,
                          int n1, const uint8_t* desc1, const orb_keypoint* kps1, const float* centres,
                          float window, int n2, const uint8_t* desc2, const orb_keypoint* kps2,
                          orb_frame_grid grid2, int* match12, int* nmatches);

/* The projection-gated searches of the tracking thread, one generic core: each query (a projected map point) has
 * a descriptor (qdesc, 32 B each), a window centre (u, v) and final radius r in the train frame, the
 * GetFeaturesInArea level arguments with the reference's semantics (Frame.cc:515-527: levels are checked when
 * min_level > 0 || max_level >= 0; then octave < min_level is skipped, and octave > max_level when max_level >= 0),
 * and the stereo values.  Trains are the Frame's features: tdesc, kps_t (mvKeysUn / mvKeysBird), t_uright
 * (mvuRight; NULL = mono / birdview: no stereo gate), t_taken[t] != 0 <=> mvpMapPoints[t] && Observations() > 0
 * (NULL = none), and the Frame's grid (orb_frame_grid; the birdview grid for the birdview form).  Candidates =
 * GetFeaturesInArea(u, v, r, min_level, max_level) computed on the GPU, minus taken trains, minus trains with
 * uright > 0 && fabsf(ur - uright) > ur_tol (ORBmatcher.cc:91-96, :1407-1413).  The acceptance runs in query order:
 * a train assigned to a query with blocks != 0 is taken for the queries after it; one assigned to a query with
 * blocks == 0 (a MapPoint without observations, e.g. the temporal points of Tracking::UpdateLastFrame) may be
 * assigned again, and *nmatches counts both assignments as the reference does.
 *   ORB_PROJ_BEST (:1397-1442): the smallest distance (first on ties) is accepted when <= max_dist; with check_ori
 *     the rotation histogram over q.angle - kps_t[best].angle and the ComputeThreeMaxima cull (:1448-1467).
 *   ORB_PROJ_RATIO_SAME_LEVEL (:76-125, :1952-1994): best and second best with their octaves; accepted when
 *     best <= max_dist unless bestLevel == bestLevel2 && best > nnratio * best2.  check_ori is not read.
 * match_t[t] (nt ints) = the last query assigned to train t, -1 = untouched, -2 = reset to NULL by the rotation
 * cull; *nmatches = the reference function's return value.  How the reference calls map onto it (points the
 * reference skips before its search are left out by the caller: outliers, !mbTrackInView, isBad, invzc < 0,
 * projections out of bounds, mnLastFrameSeen == F.mnId, |z| > 0.2):
 *   SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)   ORBmatcher.cc:1328-1470
 *     (u, v) the projection (:1370-1371), r = th * mvScaleFactors[octave] (:1381); levels (octave, -1) if bForward,
 *     (0, octave) if bBackward, else (octave - 1, octave + 1) (:1385-1390); ur = u - mbf * invzc, ur_tol = r;
 *     angle = LastFrame.mvKeysUn[i].angle; blocks = pMP->Observations() > 0; mode BEST, max_dist TH_HIGH.
 *   SearchByProjection(Frame& F, const vector<MapPoint*>&, th)                   ORBmatcher.cc:45-129
 *     (u, v) = (mTrackProjX, mTrackProjY), r = RadiusByViewingCos(mTrackViewCos) [* th if th != 1] *
 *     mvScaleFactors[mnTrackScaleLevel] (:63-69); levels (level - 1, level); ur = mTrackProjXR, ur_tol = r;
 *     blocks = 1; mode RATIO_SAME_LEVEL, max_dist TH_HIGH.
 *   SearchByProjectionBird(Frame& F, const vector<MapPointBird*>&, r)            ORBmatcher.cc:1923-1998
 *     (u, v) = pt (:1940), the given r; levels (-1, -1); t_uright NULL; blocks = 1; mode RATIO_SAME_LEVEL,
 *     max_dist TH_HIGH; kps_t = mvKeysBird, tdesc = mDescriptorsBird, t_taken from mvpMapPointsBird, the birdview grid.
 * ORB_ERR_ARG before any GPU work: an unknown mode, a u, v or r that is not finite, r < 0, max_dist outside
 * [0, 256], a grid CSR orb_window_match_grid would refuse.  nq == 0 or nt == 0: ORB_OK, *nmatches = 0, match_t all
 * -1, no GPU work. */
enum { ORB_PROJ_BEST = 0, ORB_PROJ_RATIO_SAME_LEVEL = 1 };
typedef struct orb_proj_query {
    float u, v, r;              /* window centre and final radius (th * scale already applied) */
    int   min_level, max_level; /* GetFeaturesInArea's arguments, reference semantics */
    float ur, ur_tol;           /* projected right coordinate and its tolerance */
    float angle;                /* query keypoint angle (BEST + check_ori) */
    int   blocks;               /* the query's MapPoint has Observations() > 0 */
} orb_proj_query;
int orb_search_by_projection(orb_ctx* ctx, int mode, float nnratio, int check_ori, int max_dist,
                             int nq, const orb_proj_query* q, const uint8_t* qdesc,
                             int nt, const uint8_t* tdesc, const orb_keypoint* kps_t, const float* t_uright,
                             const uint8_t* t_taken, orb_frame_grid grid, int* match_t, int* nmatches);
/* The keyframe forms of SearchByProjection map onto the same core (points the reference skips before its search are
 * left out by the caller: isBad, already found, negative depth, !IsInImage, the distance and viewing-angle tests):
 *   SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>& vpMatched, th)  :290-403
 *     r = th * mvScaleFactors[nPredictedLevel]; levels (pred - 1, pred); t_uright NULL; blocks = 1;
 *     t_taken[idx] = vpMatched[idx] != NULL; mode BEST, check_ori 0, max_dist TH_LOW.
 *   SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>&, th, ORBdist)                  :1472-1599
 *     r = th * mvScaleFactors[nPredictedLevel]; levels (pred - 1, pred + 1); t_uright NULL; blocks = 1;
 *     angle = pKF->mvKeysUn[i].angle; t_taken[i2] = CurrentFrame.mvpMapPoints[i2] != NULL; mode BEST, the matcher's
 *     check_ori (the cull of :1577-1596 is that of :1448-1467), max_dist ORBdist. */

/* int ORBmatcher::SearchByMatchBird(KeyFrame* pKF, Frame& F, vector<MapPointBird*>& vpMapPointMatchesBird, r)
 *     ORBmatcher.cc:2000-2114 (Tracking::TrackReferenceKeyFrame, Tracking.cc:1046 / :1049).
 * Queries = the keyframe's birdview keypoints k whose MapPointBird* is not NULL (the caller leaves the others out):
 * q_id[i] = k (NULL: q_id[i] = i), q_xy[2 i], q_xy[2 i + 1] = pKF->mvKeysBird[k].pt, q_angle[i] = mvKeysBird[k].angle
 * (NULL with check_ori == 0), qdesc = the map point's GetDescriptor() (32 B each); one radius r for all.  Trains =
 * F.mvKeysBird / mDescriptorsBird with the birdview grid.  Candidates = GetFeaturesInAreaBirdview(x, y, r) without
 * level arguments (Frame.cc:891-945), computed on the GPU in the grid's order and ranked there (k_projection_topk, as
 * orb_search_by_projection); the acceptance is replayed on the host in query order, line for line:
 *   a candidate with vMatchedDistanceBird[idx] <= dist is skipped (:2051); best and second best start at INT_MAX and
 *   update on '<' only, with their octaves (bestLevel2 starts at -1; a distance of 256 is a legitimate second best);
 *   accepted when bestDist <= max_dist && (bestLevel != bestLevel2 || bestDist < (float)bestDist2 * nnratio) (:2070-2072,
 *   with (float)INT_MAX * nnratio when there is no second); then match_t[bestIdx] = q_id[i],
 *   vMatchedDistanceBird[bestIdx] = bestDist, nmatches++ (never decremented when an earlier owner is overwritten), and
 *   with check_ori bestIdx enters rotHist[bin(q_angle[i] - kps_t[bestIdx].angle)];
 *   the cull (:2093-2111): every entry of a bin outside the three maxima sets its train to -2 and decrements nmatches
 *   (no guard: a train entered twice counts twice, and is culled even if its last owner's bin is kept).
 * match_t[t] (nt ints) = the last owning q_id, -1 = untouched, -2 = reset by the cull; *nmatches = the reference's
 * return value (it can differ from the number of non-negative entries, in either direction).
 * ORB_ERR_ARG before the context is touched or any output is written: a centre or r that is not finite, r < 0,
 * max_dist outside [0, 256], NULL arrays with non-zero counts, a grid CSR orb_window_match_grid would refuse.
 * nq == 0 or nt == 0: ORB_OK, *nmatches = 0, match_t all -1, no GPU work. */
int orb_search_by_match_bird(orb_ctx* ctx, float nnratio, int check_ori, int max_dist, float r,
                             int nq, const int* q_id, const float* q_xy, const float* q_angle, const uint8_t* qdesc,
                             int nt, const uint8_t* tdesc, const orb_keypoint* kps_t, orb_frame_grid grid,
                             int* match_t, int* nmatches);
/* int ORBmatcher::SearchByMatchBird(Frame& CurrentFrame, const Frame& LastFrame, windowSize)   ORBmatcher.cc:1901-1921
 *     (Tracking::TrackWithMotionModel, Tracking.cc:1241 / :1245).
 * BirdviewMatch(LastFrame, CurrentFrame, vnMatches12, windowSize) (:1790-1899) = orb_window_match_grid with centres =
 * NULL and level0_only = 0 over CurrentFrame's birdview grid, one GPU call; then on the host, for each k with
 * vnMatches12[k] >= 0 and has_mp_last[k] != 0 (LastFrame.mvpMapPointsBird[k] != NULL): match_cur[vnMatches12[k]] = k.
 * match_cur: n_cur ints, -1 = untouched; *nmatches = the carried points (not BirdviewMatch's return value).
 * has_mp_last == NULL: no point carries a map point (0, all -1).  Arguments are checked as orb_window_match_grid's.
 * ("_frame" here names the form between two Frames; the keyframe form over a resident orb_frame handle is
 * orb_search_by_match_bird_resident.) */
int orb_search_by_match_bird_frame(orb_ctx* ctx, float nnratio, int check_ori, float window,
                                   int n_last, const uint8_t* desc_last, const orb_keypoint* kps_last,
                                   const uint8_t* has_mp_last, int n_cur, const uint8_t* desc_cur,
                                   const orb_keypoint* kps_cur, orb_frame_grid grid_cur, int* match_cur, int* nmatches);

/* The searches that decide every projected point on its own (nothing like a taken set is read inside the search):
 * Fuse(KeyFrame*, const vector<MapPoint*>&, th) (ORBmatcher.cc:823-975, gate FUSE), Fuse(KeyFrame*, cv::Mat Scw, ...)
 * (:977-1100, gate NONE) and both directions of SearchBySim3 (:1102-1326, gate NONE).  Many targets (keyframes with
 * their projected points) go into one call: one staging, one launch, one synchronisation.  Per query of a target the
 * candidates are KeyFrame::GetFeaturesInArea(u, v, r) (KeyFrame.cc:586-625: Frame::GetFeaturesInArea without level
 * arguments) over the target's grid, filtered by (min_level, max_level) with orb_proj_query's semantics (the callers
 * pass (pred - 1, pred): `kpLevel<nPredictedLevel-1 || kpLevel>nPredictedLevel`), and with gate FUSE by the
 * chi-square reprojection test of :914-938: ex = u - kp.x, ey = v - kp.y, er = ur - uright[t];
 *   uright[t] >= 0 (not > 0):  skipped when (double)(e2 * inv_sigma2[octave]) > 7.8,  e2 = ex*ex + ey*ey + er*er
 *   otherwise:                 skipped when (double)(e2 * inv_sigma2[octave]) > 5.99, e2 = ex*ex + ey*ey
 * in float with the reference build's contractions (tools/fuse_flags_probe.cpp): e2 = fmaf(er, er, fmaf(ex, ex,
 * ey * ey)) and fmaf(ex, ex, ey * ey).  best_idx / best_dist[i] = the train with the smallest descriptor distance,
 * the first in candidate order on ties, and that distance; -1 / -1 if no candidate passes.  TH_LOW / TH_HIGH and
 * what follows (GetMapPoint, Replace, AddObservation, the Sim3 agreement) are the caller's.
 * ORB_ERR_ARG before any GPU work, and nothing runs if any target is malformed: an unknown gate, ntargets < 0, NULL
 * outputs with nq > 0, a u, v or r that is not finite or r < 0, with gate FUSE a ur that is not finite, a grid CSR
 * orb_window_match_grid would refuse, gate FUSE with inv_sigma2 == NULL, nlevels outside [1, ORBGPU_MAX_LEVELS] or a
 * train octave outside [0, nlevels).  ntargets == 0, a target with nq == 0: ORB_OK; nt == 0: its outputs are -1. */
enum { ORB_PROJ_GATE_NONE = 0, ORB_PROJ_GATE_FUSE = 1 };
typedef struct orb_proj_target {
    int nq; const orb_proj_query* q; const uint8_t* qdesc;   /* u, v, r, min_level, max_level, ur are read;
                                                                 ur_tol, angle, blocks are ignored */
    int nt; const uint8_t* tdesc; const orb_keypoint* kps_t; /* mvKeysUn, mDescriptors of the keyframe */
    const float* t_uright;      /* mvuRight; NULL = every train is monocular (gate FUSE only) */
    const float* inv_sigma2;    /* mvInvLevelSigma2, nlevels entries (gate FUSE only) */
    int nlevels;
    orb_frame_grid grid;        /* the keyframe's mGrid, as for orb_search_by_projection */
    int* best_idx; int* best_dist;   /* nq each: first minimum in GetFeaturesInArea order; -1 / -1 if none passes */
} orb_proj_target;
int orb_project_best_batch(orb_ctx* ctx, int gate, int ntargets, const orb_proj_target* targets);
/* One query of one target on the CPU (host only, no context): the same arithmetic and the same result as
 * orb_project_best_batch gives for it, for a caller that replays a point whose descriptor changed after the batched
 * call.  The target's best_idx / best_dist are not touched.  ORB_ERR_ARG as above, for this target
 * and this query. */
int orb_project_best_host(int gate, const orb_proj_target* target, int query, int* best_idx, int* best_dist);

/* Frame::GetFeaturesInArea over the 64x48 Frame grid (Frame.cc:378-412, 494-560): host helper the
 * C++ mirror uses to build window candidate lists. Returns count or -(needed)-1. */
int orb_features_in_area(int n, const orb_keypoint* kps_un, float min_x, float max_x, float min_y, float max_y,
                         float x, float y, float r, int min_level, int max_level, int* out, int cap);

/* ======================= Resident Frame / KeyFrame handles ======================= */

/* The train side of the grid searches, kept on the device: a Frame is searched several times within a few
 * milliseconds (SearchByProjection and its 2*th retry, SearchLocalPoints, the birdview searches) and a KeyFrame for as
 * long as it lives (Fuse from every neighbour, SearchBySim3, relocalisation, loop closing).  A handle is created once
 * from the frame's descriptors (32 B each), undistorted keypoints and, optionally, mvuRight; the library builds the
 * Frame grid on the GPU (Frame::AssignFeaturesToGrid with PosInGrid, Frame.cc:378-413, :549-559: cell (ix, iy) =
 * (round((x - min_x) * inv_w), round((y - min_y) * inv_h)) in float, half away from zero, inside iff 0 <= ix < 64 and
 * 0 <= iy < 48 compared after the rounding; each cell's indices ascend, the order of the reference's push_back loop).
 * min_x / min_y / inv_w / inv_h are orb_frame_grid's (mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv);
 * the birdview grid passes its inverses with origin 0.
 *   orb_frame_create         arrays in host memory
 *   orb_frame_create_device  arrays in device memory of the context's GPU (e.g. a slot of orb_extract_batch_device's
 *                            outputs): copied device-to-device on the context's stream, the keypoints come back to the
 *                            host once (the searches' host replays read octave and angle)
 * Both synchronise before they return; the handle is then usable with any context of the same device (another device:
 * ORB_ERR_ARG from the search), from one thread at a time per context as every call here.  It owns one device
 * allocation and must be destroyed before the context that created it.
 * ORB_ERR_ARG before any GPU work: n < 0, NULL desc / kps with n > 0, inv_w / inv_h not finite or <= 0, min_x / min_y
 * not finite, and for orb_frame_create a keypoint x or y that is not finite.  n == 0 is a valid empty frame.
 * orb_frame_grid_read copies the grid out (cell_off: 64 * 48 + 1 ints; cell_idx: *nslots <= n ints; ORB_ERR_CAPACITY
 * with *nslots set when cap is smaller). */
typedef struct orb_frame orb_frame;
typedef struct orb_vocab orb_vocab;   /* (the vocabulary section below) */
int  orb_frame_create(orb_ctx* ctx, int n, const uint8_t* desc, const orb_keypoint* kps_un, const float* uright,
                      float min_x, float min_y, float inv_w, float inv_h, orb_frame** out);
int  orb_frame_create_device(orb_ctx* ctx, int n, const uint8_t* d_desc, const orb_keypoint* d_kps,
                             const float* d_uright, float min_x, float min_y, float inv_w, float inv_h,
                             orb_frame** out);
void orb_frame_destroy(orb_frame* frame);
int  orb_frame_count(const orb_frame* frame);
int  orb_frame_grid_read(const orb_frame* frame, int* cell_off, int* cell_idx, int cap, int* nslots);

/* BoW on the handle: Frame::ComputeBoW / KeyFrame::ComputeBoW (Frame.cc:562-569, KeyFrame.cc:74-83) without the
 * descriptors leaving the device.  A handle may carry a BoW part, an allocation of its own that it owns: the
 * per-feature triples (word id, weight, node levelsup above the leaf), a per-feature node id (0xFFFFFFFF for a feature
 * outside the FeatureVector) and the FeatureVector as CSR (node ids strictly ascending, nnodes + 1 offsets, a node's
 * feature indices ascending), with a host copy of the CSR for the searches' replays.  Attaching again replaces it.
 *   orb_frame_compute_bow   transform(mDescriptors, mBowVec, mFeatVec, levelsup) (TemplatedVocabulary.h:1139-1210) for
 *                           nframes handles: one k_vocab_transform launch over all their resident descriptors, one
 *                           k_frame_featvec launch (a feature is in the FeatureVector iff (double)weight > 0, DBoW2's
 *                           "not stopped"; equal to orb_vocab_bow's fv_* for the same triples, n == 0 and an
 *                           all-stopped frame included), one synchronisation.  ORB_ERR_ARG before the context is
 *                           touched: nframes < 0, a NULL vocabulary / handle, a handle listed twice; then a vocabulary
 *                           or handle of another device.  On failure no handle is changed.
 *   orb_frame_set_featvec   attaches a FeatureVector the caller holds (a KeyFrame's mFeatVec): checked as the matchers
 *                           check an orb_featvec over the handle's n (ORB_ERR_ARG before any GPU work; node id
 *                           0xFFFFFFFF is reserved), uploaded once; synchronises.  The triples are then absent.
 *   orb_frame_has_bow       0: none, 1: a FeatureVector only, 2: with the triples.
 *   orb_frame_bow_read      the BowVector (words ascending, values in double: orb_vocab_bow's own summation over the
 *                           handle's triples, on the host; *nbow = 0 and vocab unused without triples) and the
 *                           FeatureVector from the CSR the GPU built, in orb_vocab_bow's output format (arrays of n
 *                           entries, fv_off n + 1; after orb_frame_set_featvec as many as the given CSR held).  Host
 *                           only.  ORB_ERR_ARG for a NULL handle or one without BoW. */
int orb_frame_compute_bow(orb_ctx* ctx, const orb_vocab* vocab, int levelsup, int nframes, orb_frame* const* frames);
int orb_frame_set_featvec(orb_ctx* ctx, orb_frame* frame, orb_featvec fv);
int orb_frame_has_bow(const orb_frame* frame);
int orb_frame_bow_read(const orb_vocab* vocab, const orb_frame* frame, int* bow_words, double* bow_values, int* nbow,
                       uint32_t* fv_nodes, int* fv_off, int* fv_idx, int* nfv);

/* The vocabulary-gated searches between handles that carry BoW: every output and the return value are byte for byte
 * those of the host-pointer entry point on the same data (the handles' descriptors, keypoints, uright and
 * FeatureVectors), and nothing per feature is staged: the only per-call upload is the map-point flags (and a small
 * table of per-keyframe constants).  ORB_ERR_ARG before the context is touched: a NULL handle, a handle without BoW,
 * handles of different devices or of another device than the context's, a NULL output, NULL flags with n > 0, a
 * negative count.  One launch sequence and one synchronisation per call (one more per re-rank of the BoW searches, as
 * in the host-pointer forms).
 *   orb_search_for_triangulation_frames  = orb_search_for_triangulation_batch (LocalMapping::CreateNewMapPoints,
 *     LocalMapping.cc:247-278): frame1 against pairs[p].frame2, one wavefront per (pair, KF1 feature)
 *     (k_triangulation_frames).  Both sides must have been created with uright (ORB_ERR_ARG otherwise); frame1's
 *     FeatureVector must list no feature twice (one built by orb_frame_compute_bow never does); nlevels2 outside
 *     [1, ORBGPU_MAX_LEVELS] or a frame2 keypoint octave outside [0, nlevels2) is ORB_ERR_ARG; at most 65535 pairs.
 *     ORB_ERR_CAPACITY as the batch call: every *npairs holds its full count.
 *   orb_search_by_bow_frames_kf_f   = orb_search_by_bow_kf_f_batch (Tracking::TrackReferenceKeyFrame,
 *     Tracking.cc:766-772, and Relocalization, :1931-1938): keyframe kfs[p].frame with its map-point flags mp against
 *     the Frame frame_f; match: frame_f's n ints.  The items are built on the device (k_bow_items).
 *   orb_search_by_bow_frames_kf_kf  = orb_search_by_bow_kf_kf (one KF2; loop closing's callers loop over it). */
typedef struct orb_tri_frame_pair {
    const orb_frame* frame2;
    const uint8_t* has_mp2;
    const float* F12;            /* row-major 3x3 */
    float ex, ey;
    const float* scale2;         /* pKF2->mvScaleFactors, nlevels2 entries */
    const float* sigma2_2;       /* pKF2->mvLevelSigma2 */
    int nlevels2;
    int* pairs_out;              /* 2 ints per pair */
    int cap;
    int* npairs;
} orb_tri_frame_pair;
int orb_search_for_triangulation_frames(orb_ctx* ctx, int check_ori, int only_stereo, const orb_frame* frame1,
                                        const uint8_t* has_mp1, int npairs, const orb_tri_frame_pair* pairs);
typedef struct orb_bow_frame_kf {
    const orb_frame* frame;
    const uint8_t* mp;
    int* match;
    int* nmatches;
} orb_bow_frame_kf;
int orb_search_by_bow_frames_kf_f(orb_ctx* ctx, float nnratio, int check_ori, const orb_frame* frame_f, int nkf,
                                  const orb_bow_frame_kf* kfs);
int orb_search_by_bow_frames_kf_kf(orb_ctx* ctx, float nnratio, int check_ori, const orb_frame* kf1, const uint8_t* mp1,
                                   const orb_frame* kf2, const uint8_t* mp2, int* match12, int* nmatches);

/* The grid searches with a handle as their train side: every output is byte for byte that of the host-pointer entry
 * point given the same train data and a grid equal to the handle's, and every argument check of that entry point
 * applies (before the context is touched or any output is written); a NULL handle or one of another device is
 * ORB_ERR_ARG.  Nothing of the train side is staged or uploaded.  nq == 0 (n1 == 0) or an empty frame: ORB_OK, the
 * outputs -1 and 0, no GPU work.
 *   orb_search_by_projection_frame  = orb_search_by_projection; use_uright = 0 is t_uright == NULL (mono, birdview,
 *     the keyframe forms), use_uright = 1 gates on the handle's uright (ORB_ERR_ARG if it was created without).
 *   orb_window_match_frame          = orb_window_match_grid with F2 as a handle.
 *   orb_search_by_match_bird_resident = orb_search_by_match_bird, the KEYFRAME form (queries = map points of a
 *     keyframe, trains = the Frame's birdview features, here a handle over mvKeysBird / mDescriptorsBird and the
 *     birdview grid).  Not to be confused with orb_search_by_match_bird_frame, the form between two Frames
 *     (SearchByMatchBird(CurrentFrame, LastFrame, windowSize)), which takes host arrays.
 *   orb_project_best_frames         = orb_project_best_batch with each target's trains as a handle (gate FUSE reads
 *     the handle's uright if it has one; inv_sigma2 / nlevels stay per target). */
int orb_search_by_projection_frame(orb_ctx* ctx, int mode, float nnratio, int check_ori, int max_dist,
                                   int nq, const orb_proj_query* q, const uint8_t* qdesc, const orb_frame* frame,
                                   const uint8_t* t_taken, int use_uright, int* match_t, int* nmatches);
int orb_window_match_frame(orb_ctx* ctx, float nnratio, int check_ori, int level0_only,
                           int n1, const uint8_t* desc1, const orb_keypoint* kps1, const float* centres,
                           float window, const orb_frame* frame2, int* match12, int* nmatches);
int orb_search_by_match_bird_resident(orb_ctx* ctx, float nnratio, int check_ori, int max_dist, float r,
                                      int nq, const int* q_id, const float* q_xy, const float* q_angle,
                                      const uint8_t* qdesc, const orb_frame* frame, int* match_t, int* nmatches);
typedef struct orb_proj_frame_target {
    int nq; const orb_proj_query* q; const uint8_t* qdesc;   /* as orb_proj_target's */
    const orb_frame* frame;     /* the keyframe */
    const float* inv_sigma2;    /* mvInvLevelSigma2, nlevels entries (gate FUSE only) */
    int nlevels;
    int* best_idx; int* best_dist;
} orb_proj_frame_target;
int orb_project_best_frames(orb_ctx* ctx, int gate, int ntargets, const orb_proj_frame_target* targets);

/* ======================= UndistortKeyPoints / ComputeImageBounds; resident frames from an extraction ============= */

/* Frame::UndistortKeyPoints (Frame.cc:571-603) and Frame::ComputeImageBounds (Frame.cc:605-660), which in this fork
 * call cv::fisheye::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK).  The definition is OpenCV 3.2 fisheye.cpp
 * on x86-64 without FMA, in double: fx, fy, cx, cy are mK's floats, k[0..3] mDistCoef's four floats in
 * the order Tracking.cc:68-72 stores them (Camera.k1, k2, p1, p2), which the fisheye model reads as k1..k4.
 * k[0] == 0.0f is the reference's identity path whatever k[1..3] hold: positions come back bit for bit, the bounds are
 * 0, w, 0, h.  A NaN result is stored as 0x7FC00000 (the one decided deviation: NaN payloads differ between libms); an
 * infinite one keeps its sign.  Only x and y of a keypoint change; its other 24 bytes are copied.
 *   orb_undistort_points_host  the definition, on the CPU (std::tan): n (x, y) pairs in, n pairs out (xy_un may be xy).
 *                              No context, no GPU.  Positions that are not finite go through the arithmetic.
 *   orb_image_bounds           mnMinX, mnMaxX, mnMinY, mnMaxY of a w x h image: the four corners through the same
 *                              function and the reference's loop, whose maxima start at numeric_limits<float>::min()
 *                              (the smallest positive float: a maximum that would be negative or zero stays there).
 *                              No context, no GPU.
 *   orb_undistort_keypoints    n keypoints in host arrays, undistorted on the GPU (kps_un may be kps).
 *   orb_undistort_keypoints_device  a whole batch in orb_extract_batch_device's output layout (frame f's records at
 *                              d_kps + f * kp_cap, its count in d_counts[f]) in one launch; d_kps_un has the same
 *                              layout and may be d_kps; slots past a frame's count are not written.
 * The GPU forms return exactly the bytes of orb_undistort_points_host: the kernel computes each result from its own
 * tan and from both ends of a guard band around it, and the few points whose results differ (a few coordinates in
 * 10^7) are recomputed by the host function before the call returns; *n_redone (may be NULL) receives their number.
 *   orb_frame_create_from_extract  orb_frame_create_device for RAW keypoints: one frame's descriptors, raw keypoints
 *                              and optionally uright in device memory (e.g. a slot of orb_extract_batch_device's
 *                              outputs) become a resident frame whose keypoints (device and host copy) are the
 *                              undistorted ones; the grid is built from them.  The inputs are not modified.
 *   orb_frames_create_from_batch   the same for nframes frames in orb_extract_batch_device's output layout (no
 *                              uright): one undistort launch, one grid launch per frame, the stream synchronised
 *                              three times whatever nframes is.  out receives nframes handles (an empty frame gets an
 *                              empty handle); on any failure none is leaked and out is untouched.  A count above
 *                              kp_cap is ORB_ERR_CAPACITY.
 * All GPU forms return synchronised, on the context's stream, and follow orb_frame_create_device's rules for device,
 * thread and lifetime.  ORB_ERR_ARG before any GPU work, outputs untouched: dist NULL; fx or fy zero or not finite;
 * cx, cy or a k not finite; n or nframes negative (nframes above 65,535, nframes * kp_cap above INT_MAX); NULL arrays
 * with n > 0 (nframes > 0); kp_cap < 1 with nframes > 0; orb_frame_create's grid checks; negative w or h; and for
 * orb_undistort_keypoints a position that is not finite (positions in device arrays are not checked: they go through
 * the arithmetic, and the grid leaves out a keypoint whose undistorted position is not finite).  n == 0 / nframes == 0
 * is ORB_OK without a context, except that orb_frame_create_from_extract with n == 0 creates an empty handle.
 *   orb_debug_undistort_guard  the guard band's relative half-width g for this context (0 restores the default,
 *                              2^-46; below the default the equality with the host function is no longer assured). */
typedef struct orb_distortion { float fx, fy, cx, cy; float k[4]; } orb_distortion;
int orb_undistort_points_host(const orb_distortion* dist, int n, const float* xy, float* xy_un);
int orb_image_bounds(const orb_distortion* dist, int w, int h, float* min_x, float* max_x, float* min_y, float* max_y);
int orb_undistort_keypoints(orb_ctx* ctx, const orb_distortion* dist, int n, const orb_keypoint* kps,
                            orb_keypoint* kps_un, int* n_redone);
int orb_undistort_keypoints_device(orb_ctx* ctx, const orb_distortion* dist, int nframes, const orb_keypoint* d_kps,
                                   const int* d_counts, int kp_cap, orb_keypoint* d_kps_un, int* n_redone);
int orb_frame_create_from_extract(orb_ctx* ctx, const orb_distortion* dist, int n, const uint8_t* d_desc,
                                  const orb_keypoint* d_kps_raw, const float* d_uright, float min_x, float min_y,
                                  float inv_w, float inv_h, orb_frame** out);
int orb_frames_create_from_batch(orb_ctx* ctx, const orb_distortion* dist, int nframes, const uint8_t* d_desc,
                                 const orb_keypoint* d_kps_raw, const int* d_counts, int kp_cap, float min_x,
                                 float min_y, float inv_w, float inv_h, orb_frame** out);
int orb_debug_undistort_guard(orb_ctx* ctx, double g);

/* ======================= Resident map points: isInFrustum and Fuse's projection ======================= */

/* The query side of the projection searches, kept on the device: the same map points are projected frame after frame
 * (Tracking::SearchLocalPoints, Tracking.cc:1635-1648 -> Frame::isInFrustum, Frame.cc:436-492) and keyframe after
 * keyframe (ORBmatcher::Fuse, ORBmatcher.cc:852-890).  A handle owns slots 0 .. capacity-1; a slot holds GetWorldPos
 * (3 floats), GetNormal (3 floats), the raw mfMinDistance / mfMaxDistance (not the invariance values: the kernel
 * applies 0.8f / 1.2f) and GetDescriptor (32 B).
 *   orb_points_create    capacity >= 0 slots on ctx's device (their content is undefined until written).
 *   orb_points_write     slots first .. first+n-1 from host arrays (pos, normal: 3 n floats; min_dist, max_dist: n;
 *                        desc: 32 n bytes).  Synchronous.  Grows the handle when first + n > capacity (earlier slots keep
 *                        their content; the growth waits for the device).  A point whose descriptor, position or normal
 *                        changed (Replace, UpdateNormalAndDepth, bundle adjustment) is rewritten through this call.
 *   orb_points_capacity  slots (0 for NULL).
 * Lifetime and device rules are orb_frame's: usable with any context of the same device, one thread at a time, destroyed
 * before the context that created it.  ORB_ERR_ARG before any GPU work: a negative capacity, first or n, NULL arrays
 * with n > 0, a position, normal or distance that is not finite, first + n beyond INT_MAX. */
typedef struct orb_points orb_points;
int  orb_points_create(orb_ctx* ctx, int capacity, orb_points** out);
int  orb_points_write(orb_points* points, int first, int n, const float* pos, const float* normal,
                      const float* min_dist, const float* max_dist, const uint8_t* desc);
int  orb_points_capacity(const orb_points* points);
void orb_points_destroy(orb_points* points);

/* The pose and intrinsics the projection reads: the Frame's / KeyFrame's own members, as floats. */
typedef struct orb_camera {
    float Rcw[9];                /* mRcw / GetRotation(), row-major */
    float tcw[3];                /* mtcw / GetTranslation() */
    float Ow[3];                 /* mOw / GetCameraCenter() */
    float fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;   /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    int   nlevels;               /* mnScaleLevels */
    float log_scale_factor;      /* mfLogScaleFactor */
    float scale_factors[ORBGPU_MAX_LEVELS];   /* mvScaleFactors, nlevels entries read */
} orb_camera;

/* The projection of one point, in one of two forms.  Shared (DESIGN 3.2 has the pins):
 *   Pc_i = (float)(((double)R_i0 P0 + (double)R_i1 P1 + (double)R_i2 P2) + (double)t_i)   (OpenCV's gemm, as modelled)
 *   PO = P - Ow in float; dist = (float)sqrt(sum (double)PO_i^2); dot = sum (double)PO_i (double)n_i  (cv::norm, Mat::dot)
 *   distance gates dist < 0.8f * min_dist, dist > 1.2f * max_dist
 *   level = MapPoint::PredictScale (MapPoint.cc:385-417): ratio = max_dist / dist, ceil(logf(ratio) / log_scale_factor)
 *     clamped to [0, nlevels - 1], computed on the device as the number of per-level thresholds ratio reaches; the
 *     thresholds come from the host's own logf (a ratio that is not finite gives level 0).
 * ORB_FRUSTUM_FRAME (Frame::isInFrustum; the search radius of SearchByProjection(Frame&, vector<MapPoint*>, th),
 *   ORBmatcher.cc:63-69): PcZ < 0.0f rejects; invz = 1.0f / PcZ; u = fmaf(fx * PcX, invz, cx), v likewise; u < min_x ||
 *   u > max_x (v likewise) rejects; the distance gates; view_cos = (float)(dot / (double)dist) < view_cos_limit rejects;
 *   ur = fmaf(-mbf, invz, u); r = (view_cos > 0.998 ? 2.5f : 4.0f) [* th if th != 1.0f] * scale_factors[level].
 * ORB_FRUSTUM_FUSE (Fuse(KeyFrame*, vector<MapPoint*>, th)): PcZ < 0.0f rejects; invz = 1 / PcZ; x = PcX * invz, y
 *   likewise; u = fmaf(fx, x, cx), v likewise; KeyFrame::IsInImage u >= min_x && u < max_x && v >= min_y && v < max_y;
 *   ur = fmaf(-mbf, invz, u); the distance gates; dot < 0.5 * (double)dist rejects; r = th * scale_factors[level].
 *   view_cos_limit is not read and view_cos stays 0.
 * verdict: 0 visible, 1 depth, 2 bounds, 3 distance, 4 angle, in the reference's order of tests, and 5: every test
 * passed but u, v, ur or r is not finite (PcZ == 0; the reference goes on into undefined casts there: DESIGN 3.3).  A
 * record holds what the reference had computed when it rejected; the other fields are 0 and level -1 (verdict 5 comes
 * last: its record is complete). */
enum { ORB_FRUSTUM_FRAME = 0, ORB_FRUSTUM_FUSE = 1 };
enum { ORB_POINT_VISIBLE = 0, ORB_POINT_DEPTH = 1, ORB_POINT_BOUNDS = 2, ORB_POINT_DISTANCE = 3, ORB_POINT_ANGLE = 4,
       ORB_POINT_NOT_FINITE = 5 };
typedef struct orb_point_proj {
    float u, v, ur, invz, dist, view_cos, r;
    int   level, verdict;
} orb_point_proj;

/* The entry points.  ids: n slot ids, in any order, repeats allowed.  ORB_ERR_ARG before the context is touched or
 * any output is written: a NULL handle or one of another device, negative counts, NULL arrays with non-zero counts, an
 * id outside [0, capacity), an unknown mode, a camera field that is not finite, nlevels outside [1, ORBGPU_MAX_LEVELS],
 * log_scale_factor <= 0, th or view_cos_limit not finite, th < 0, and everything the underlying search refuses.  n == 0
 * or an empty frame: ORB_OK, the outputs as the underlying search leaves them, no GPU work.
 *   orb_project_points       the projection alone: proj_out[i] for ids[i].
 *   orb_project_points_host  the same records on the CPU from host arrays indexed by i (no context, no handle): the
 *                            arithmetic of the kernel, for a caller that replays single points.
 *   orb_search_local_points  Tracking::SearchLocalPoints' isInFrustum loop and SearchByProjection(Frame&,
 *                            vector<MapPoint*>, th) in one call: the projection (FRAME), the projection top-k over the
 *                            resident frame and the host replay, nothing of the query side staged.  The outputs equal
 *                            orb_search_by_projection_frame(ORB_PROJ_RATIO_SAME_LEVEL, max_dist = TH_HIGH = 100) fed with
 *                            the visible points in ids order, every query built as orbgpu.h maps that search (levels
 *                            (level - 1, level), ur_tol = r, blocks = 1); match_t[t] holds positions in ids.  Rejected
 *                            points stay in the launch with an empty window.  proj_out may be NULL.  The caller leaves
 *                            out what the reference skips before isInFrustum (isBad, mnLastFrameSeen == mnId).
 *   orb_fuse_search_points   Fuse(KeyFrame*, vector<MapPoint*>, th) for many target keyframes in one launch: per
 *                            target the projection (FUSE) of its ids through its camera, then the search of
 *                            orb_project_best_frames(ORB_PROJ_GATE_FUSE) with levels (level - 1, level): best_idx /
 *                            best_dist as that call gives them for the visible points, -1 / -1 for the others.  proj_out
 *                            may be NULL.  isBad, IsInKeyFrame, TH_LOW and the dirty-descriptor replay
 *                            (orb_project_best_host) stay the caller's. */
int orb_project_points(orb_ctx* ctx, const orb_points* points, int mode, const orb_camera* camera, float view_cos_limit,
                       float th, int n, const int* ids, orb_point_proj* proj_out);
int orb_project_points_host(int mode, const orb_camera* camera, float view_cos_limit, float th, int n, const float* pos,
                            const float* normal, const float* min_dist, const float* max_dist, orb_point_proj* proj_out);
int orb_search_local_points(orb_ctx* ctx, const orb_points* points, const orb_camera* camera, float view_cos_limit,
                            float th, float nnratio, int n, const int* ids, const orb_frame* frame,
                            const uint8_t* t_taken, int use_uright, int* match_t, int* nmatches,
                            orb_point_proj* proj_out);
typedef struct orb_fuse_points_target {
    orb_camera camera;          /* the keyframe's pose and intrinsics */
    const orb_frame* frame;     /* the keyframe */
    const float* inv_sigma2;    /* mvInvLevelSigma2, camera.nlevels entries */
    float th;
    int n; const int* ids;      /* the points projected into this keyframe */
    int* best_idx; int* best_dist;   /* n each */
    orb_point_proj* proj_out;   /* n records, or NULL */
} orb_fuse_points_target;
int orb_fuse_search_points(orb_ctx* ctx, const orb_points* points, int ntargets,
                           const orb_fuse_points_target* targets);

/* ======================= Frame::ComputeStereoMatches ======================= */

/* The descriptor search keeps its running best as dist << 24 | right index: at most this many right keypoints
 * (nR of orb_compute_stereo_matches, kp_cap of the batch behind orb_stereo_batch_device); more is ORB_ERR_ARG. */
#define ORB_STEREO_MAX_RIGHT ((1 << 24) - 1)

/* void Frame::ComputeStereoMatches()  Frame.cc:662-836, for one rectified pair.  `left` / `right` are
 * the contexts that extracted the left / right image last (orb_extract; the reference's
 * mpORBextractorLeft/Right, whose mvImagePyramid the window search reads), same image size.  They may sit
 * on different GPUs (one GPU per camera stream): the right image and pyramid are then copied to the left
 * device with hipMemcpyPeerAsync and the search runs there.  kpsL/descL = mvKeys/mDescriptors (nL),
 * kpsR/descR = mvKeysRight/mDescriptorsRight (nR);
 * mb = baseline, mbf = baseline * fx.  uright / depth (nL each) receive mvuRight / mvDepth
 * (-1 = no match); *nmatched = number of left keypoints with a depth.  nR <= ORB_STEREO_MAX_RIGHT.  Synchronous. */
int orb_compute_stereo_matches(orb_ctx* left, orb_ctx* right, int nL, const orb_keypoint* kpsL, const uint8_t* descL,
                               int nR, const orb_keypoint* kpsR, const uint8_t* descR, float mb, float mbf,
                               float* uright, float* depth, int* nmatched);

/* Device-resident batched form: frames (2p, 2p+1) of the last orb_extract_batch_device on ctx are
 * the (left, right) images of pair p.  Outputs at d_uright/d_depth[p * kp_cap + i] (kp_cap of that
 * batch) and d_nmatched[p].  kp_cap <= ORB_STEREO_MAX_RIGHT.  Asynchronous on the context stream. */
int orb_stereo_batch_device(orb_ctx* ctx, int npairs, float mb, float mbf, float* d_uright, float* d_depth,
                            int* d_nmatched);

/* ======================= Colour input: cvtColor to gray (Tracking::GrabImage*) ======================= */

/* The first lines of Tracking::GrabImageStereo / RGBD / Monocular / MonocularWithBirdview (Tracking.cc:172-198,
 * :212-230, :242-257, :276-307): cvtColor(im, mImGray, CV_RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY), for the left,
 * right and birdview images alike.  The definition is OpenCV 3.2 RGB2Gray<uchar> on x86-64 without IPP (DESIGN.md
 * §3.3):  Y = (4899 R + 9617 G + 1868 B + 8192) >> 14;  alpha is ignored.  There is no variant bit for it.
 * Pixels are interleaved 8-bit, 3 or 4 bytes each in the order the code names; rows are src_stride / dst_stride bytes
 * apart; any base alignment and any stride (multiples of 4 or not) are accepted.  Only [row, row + w * channels) of
 * the source is read and only [row, row + w) of the destination written: padding bytes stay untouched.
 *   orb_to_gray_host    the definition, on the CPU.  No context, no GPU.
 *   orb_to_gray_device  nframes frames in device memory in one launch (k_to_gray), asynchronous on the context's
 *                       stream: frame f at d_src + f * src_frame_pitch -> d_dst + f * dst_frame_pitch.  d_dst is what
 *                       orb_extract_batch_device consumes (same stream: no synchronisation in between).  The birdview
 *                       object has a STREAM OF ITS OWN: call orb_sync before d_dst goes to orb_bird_extract_device or
 *                       orb_bird_extract_batch_device.
 *   orb_extract_color   orb_extract for a host colour image: the colour image is uploaded, converted on the device and
 *                       goes through orb_extract's single-frame chain unchanged.  orb_get_level(ctx, 0, ...) afterwards
 *                       returns the gray image (mImGray).  Empty image (w == 0 || h == 0 || img == NULL): ORB_OK, the
 *                       outputs untouched; capacity as orb_extract.
 * ORB_ERR_ARG before any GPU work, outputs untouched: an unknown code; NULL arrays with a non-empty image; a negative
 * size or nframes; a source stride below w * channels or a destination stride below w; a side above 4096; with
 * nframes > 1 a frame pitch below (h - 1) * stride + the row's bytes.  nframes == 0, w == 0 or h == 0: ORB_OK,
 * nothing touched. */
enum { ORB_COLOR_RGB = 0, ORB_COLOR_BGR = 1, ORB_COLOR_RGBA = 2, ORB_COLOR_BGRA = 3 };
int orb_to_gray_host(int code, const uint8_t* src, int w, int h, size_t src_stride, uint8_t* dst, size_t dst_stride);
int orb_to_gray_device(orb_ctx* ctx, int code, const uint8_t* d_src, int nframes, int w, int h, size_t src_frame_pitch,
                       size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch, size_t dst_row_stride);
int orb_extract_color(orb_ctx* ctx, int code, const uint8_t* img, int w, int h, size_t stride, orb_keypoint* kps,
                      int cap, int* n, uint8_t* desc);

/* ======================= Frame::ComputeStereoFromRGBD (the RGB-D Frame constructor) ======================= */

/* void Frame::ComputeStereoFromRGBD(const cv::Mat& imDepth)  Frame.cc:839-860, with Tracking::GrabImageRGBD's
 * imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (Tracking.cc:229-230) folded in.  For keypoint i:
 *   col = (int)kp.pt.x, row = (int)kp.pt.y of the RAW keypoint (Mat::at<float>(float, float) truncates toward zero);
 *   d = (float)depth[row][col] * factor            (convertTo's float work type with beta 0: one rounding);
 *   d > 0:  mvDepth[i] = d,  mvuRight[i] = kpU.pt.x - mbf / d   (the UNDISTORTED x; the float division first);
 *   else:   both stay -1.  NaN, 0, -0 and negatives fail d > 0; +inf passes and gives uright = kpU.pt.x.
 * The converted image is never materialised: only the n gathered values are converted, each bit-equal to the converted
 * image's value, so a raw 16-bit map goes up at 2 bytes per pixel.  A CV_32F map with factor 1 is the same expression.
 * THE ONE DECIDED DEVIATION: the reference indexes outside the image by undefined behaviour only.  Here a keypoint
 * whose raw position is not finite or truncates outside [0, w) x [0, h) gets -1 / -1 in the device forms, and is
 * ORB_ERR_ARG (outputs untouched) in the host-array form.
 *   orb_stereo_from_rgbd_host    the definition, on the CPU, map and keypoints in host memory; no context, no GPU.  It
 *                                is also the right call for ONE frame whose keypoints are already on the host:
 *                                uploading a depth map to gather a thousand values is not a win.
 *   orb_stereo_from_rgbd_device  a batch in orb_extract_batch_device's output layout, everything in device memory:
 *                                frame f's map at map->data + f * map->frame_pitch, its raw / undistorted keypoints at
 *                                d_kps_raw / d_kps_un + f * kp_cap (they may be the same array), its count in
 *                                d_counts[f]; outputs at d_uright / d_depth[f * kp_cap + i], d_nvalid[f] = keypoints
 *                                with a depth (d_nvalid may be NULL).  One launch (k_rgbd_depth), asynchronous on the
 *                                context's stream.  Slots past a frame's count are not written; a count above kp_cap is
 *                                read as kp_cap.
 *   orb_frames_create_from_batch_rgbd  the RGB-D Frame constructor after extraction (Frame.cc:145-200) in one call:
 *                                orb_frames_create_from_batch's undistort launch with its guard-band redo, then the
 *                                depth launch on the undistorted keypoints, then the grids; every handle carries its
 *                                uright (use_uright = 1 works).  d_uright / d_depth (nframes * kp_cap floats each, the
 *                                layout above) receive mvuRight / mvDepth; either may be NULL.  Failure, synchronisation
 *                                and argument rules are orb_frames_create_from_batch's.
 * A map's elements are aligned: data, row_stride and frame_pitch are multiples of the element size (2 or 4), as
 * cv::Mat's are.  ORB_ERR_ARG before any GPU work, outputs untouched: map NULL; an unknown type; factor or mbf not
 * finite; w or h negative or above 4096; row_stride below w * element size; with nframes > 1 a frame_pitch below
 * row_stride * h; a misaligned map; n or nframes negative; NULL arrays (map->data included) with n > 0 / nframes > 0;
 * and what orb_frames_create_from_batch refuses.  n == 0 / nframes == 0: ORB_OK (*nvalid = 0). */
enum { ORB_DEPTH_U16 = 0, ORB_DEPTH_F32 = 1 };
typedef struct orb_depth_map {
    const void* data;      /* host memory (orb_stereo_from_rgbd_host) or device memory */
    int type;              /* ORB_DEPTH_U16 | ORB_DEPTH_F32 */
    int w, h;
    size_t row_stride;     /* bytes */
    size_t frame_pitch;    /* bytes between the maps of a batch (one map: not read) */
    float factor;          /* mDepthMapFactor (Tracking.cc:144-148: already inverted, e.g. 1.0f / 5000.0f) */
} orb_depth_map;
int orb_stereo_from_rgbd_host(const orb_depth_map* map, float mbf, int n, const orb_keypoint* kps,
                              const orb_keypoint* kps_un, float* uright, float* depth, int* nvalid);
int orb_stereo_from_rgbd_device(orb_ctx* ctx, const orb_depth_map* map, float mbf, int nframes,
                                const orb_keypoint* d_kps_raw, const orb_keypoint* d_kps_un, const int* d_counts,
                                int kp_cap, float* d_uright, float* d_depth, int* d_nvalid);
int orb_frames_create_from_batch_rgbd(orb_ctx* ctx, const orb_distortion* dist, const orb_depth_map* map, float mbf,
                                      int nframes, const uint8_t* d_desc, const orb_keypoint* d_kps_raw,
                                      const int* d_counts, int kp_cap, float min_x, float min_y, float inv_w,
                                      float inv_h, float* d_uright, float* d_depth, orb_frame** out);

/* ======================= Stereo input: rectification (cv::remap) and the stereo Frame constructor ============= */

/* cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) as every stereo frame of the reference goes through it, once per eye,
 * before System::TrackStereo sees it (Examples/Stereo/stereo_euroc.cc:136-137, Examples/ROS/ORB_SLAM2/src/
 * ros_stereo.cc:161-162): 8-bit one-channel images, CV_32FC1 map1 / map2, INTER_LINEAR, BORDER_CONSTANT with value 0.
 * The definition is OpenCV 3.2 imgwarp.cpp on x86-64 without IPP, RemapInvoker + remapBilinear<FixedPtCast<int, uchar,
 * 15>, RemapVec_8u, short>.  The destination has the maps' size (dw, dh); the source (sw, sh) may
 * differ.  For a destination pixel with map values mx, my:
 *   sx = cvtss2si(mx * 32.0f), sy likewise: to nearest, ties to even; NaN, +-inf or a product outside int give INT_MIN;
 *   ix = sat_s16(sx >> 5) (arithmetic shift), fx = sx & 31; iy, fy likewise;
 *   w00 = (32-fx)(32-fy)*32, w01 = fx(32-fy)*32, w10 = (32-fx)fy*32, w11 = fx*fy*32  (integers, sum 32768);
 *   each of the taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) is decided on its own: inside [0, sw) x [0, sh) it
 *   reads the source, outside it reads 0;
 *   dst = (w00 S00 + w01 S01 + w10 S10 + w11 S11 + 16384) >> 15.
 * Rows are stride bytes apart for the images and map_stride bytes apart for the maps; any base alignment and any
 * stride are accepted for the images, maps are 4-byte aligned (base and stride).  Only [row, row + dw) of the
 * destination is written: padding bytes stay untouched.  There is no variant bit for it.
 *   orb_remap_host         the definition, on the CPU.  No context, no GPU.
 *   orb_rectify_maps_host  cv::initUndistortRectifyMap(K, D, R, P(0:3,0:3), size, CV_32F, m1, m2) of OpenCV 3.2
 *                          undistort.cpp, on the CPU, one-off per calibration.  K, R, P33: nine doubles each, row-major,
 *                          as the YAML gives them; D: nD = 4, 5 or 8 doubles (k1, k2, p1, p2, then k3, then k4..k6;
 *                          missing ones 0).  All arithmetic in double, uncontracted: iR = inverse(P33 * R) (sums in the
 *                          order k = 0, 1, 2; the 3x3 adjugate times 1.0 / det); per row i: _x = i*ir[1] + ir[2], _y =
 *                          i*ir[4] + ir[5], _w = i*ir[7] + ir[8]; per column the pixel first, then _x += ir[0], _y +=
 *                          ir[3], _w += ir[6] (sequential sums); per pixel w = 1/_w, x = _x*w, y = _y*w, r2 = x2 + y2,
 *                          kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2), xd = x kr + p1 2xy +
 *                          p2 (r2 + 2 x2), yd = y kr + p1 (r2 + 2 y2) + p2 2xy, map = (float)(fx xd + u0), (float)(fy yd
 *                          + v0).  ORB_ERR_ARG: 12 or 14 coefficients (thin-prism and tilt are out of scope), any other
 *                          nD, a zero determinant, NULL arrays, a side above 4096, misaligned maps.  A caller that has
 *                          OpenCV passes ITS OWN maps to the calls below instead: the remap contract does not depend on
 *                          this builder.
 *   orb_rectify_create     the resident map of one camera, built once: the float maps (host memory) are converted to the
 *                          fixed-point form above (OpenCV converts per call and per tile) and kept on ctx's device.
 *                          Synchronous.  Lifetime and device rules are orb_frame's: usable with any context of the same
 *                          device, one thread at a time, destroyed before the context that created it.  dw == 0 or dh ==
 *                          0 gives an empty map (every remap through it is ORB_OK with nothing touched).
 *   orb_rectify_size       the maps' (dw, dh).
 *   orb_remap_device       nframes frames in device memory in one launch (k_remap), asynchronous on the context's
 *                          stream: frame f at d_src + f * src_frame_pitch goes through maps[f % nmaps] to d_dst + f *
 *                          dst_frame_pitch.  nmaps = 1 is a mono camera; nmaps = 2 is the interleaved left / right
 *                          layout: frames 2p, 2p+1 are then exactly what orb_extract_batch_device and
 *                          orb_stereo_batch_device consume, on the same stream with no synchronisation between.  All
 *                          maps of a call have one size; at most ORB_REMAP_MAX_MAPS of them.  The birdview object has a
 *                          STREAM OF ITS OWN: call orb_sync before d_dst goes to orb_bird_extract_device.
 *   orb_remap              one host image, remapped on the GPU into a host image.  Synchronous.
 *   orb_extract_rectified  orb_extract for a raw host image: uploaded, remapped on the device, then orb_extract's
 *                          single-frame chain unchanged on the rectified image (of the maps' size).  orb_get_level(ctx,
 *                          0, ...) afterwards returns the rectified image, and two contexts that did this are valid
 *                          left / right arguments of orb_compute_stereo_matches.  Empty image (sw == 0 || sh == 0 ||
 *                          img == NULL, or an empty map): ORB_OK, the outputs untouched; capacity as orb_extract.
 * ORB_ERR_ARG before any GPU work, outputs untouched: NULL arrays with a non-empty size; negative sizes or counts; any
 * side above 4096; a stride below a row; with nframes > 1 a frame pitch below (h - 1) * stride + the row's bytes;
 * nmaps < 1 or above ORB_REMAP_MAX_MAPS, or a NULL entry; maps of differing size, or of another device than the
 * context's; float maps that are not 4-byte aligned.  nframes == 0 or an empty destination: ORB_OK, nothing touched. */
#define ORB_REMAP_MAX_MAPS 16
typedef struct orb_rectify orb_rectify;
int  orb_remap_host(const uint8_t* src, int sw, int sh, size_t src_stride, const float* map_x, const float* map_y,
                    size_t map_stride, int dw, int dh, uint8_t* dst, size_t dst_stride);
int  orb_rectify_maps_host(const double* K, const double* D, int nD, const double* R, const double* P33, int w, int h,
                           float* map_x, float* map_y, size_t map_stride);
int  orb_rectify_create(orb_ctx* ctx, int dw, int dh, const float* map_x, const float* map_y, size_t map_stride,
                        orb_rectify** out);
void orb_rectify_destroy(orb_rectify* rect);
int  orb_rectify_size(const orb_rectify* rect, int* w, int* h);
int  orb_remap_device(orb_ctx* ctx, int nmaps, const orb_rectify* const* maps, const uint8_t* d_src, int nframes, int sw,
                      int sh, size_t src_frame_pitch, size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch,
                      size_t dst_row_stride);
int  orb_remap(orb_ctx* ctx, const orb_rectify* rect, const uint8_t* img, int sw, int sh, size_t stride, uint8_t* dst,
               size_t dst_stride);
int  orb_extract_rectified(orb_ctx* ctx, const orb_rectify* rect, const uint8_t* img, int sw, int sh, size_t stride,
                           orb_keypoint* kps, int cap, int* n, uint8_t* desc);

/* The stereo Frame constructor after extraction (Frame.cc:129-141: UndistortKeyPoints, ComputeStereoMatches,
 * AssignFeaturesToGrid) in one call, after an orb_extract_batch_device of 2 * npairs frames on ctx (slots 2p, 2p+1 =
 * the left, right image of pair p; d_desc / d_kps_raw / d_counts / kp_cap are that batch's outputs):
 *   orb_frames_create_from_batch's undistort launch with its guard-band redo over the LEFT frames only (k[0] == 0 stays
 *   the identity path, which is what rectified images give); orb_stereo_batch_device's search, which reads the RAW
 *   keypoints of both sides as the reference's mvKeys / mvKeysRight; the grids of the left frames from their
 *   undistorted keypoints.
 * out receives npairs handles, every one carrying its mvuRight (use_uright = 1 works).  d_uright / d_depth (npairs *
 * kp_cap floats each, pair p's at p * kp_cap, as orb_stereo_batch_device lays them out) receive mvuRight / mvDepth;
 * either may be NULL.  Failure, synchronisation-count and argument rules are orb_frames_create_from_batch's (a count
 * above kp_cap, of a left or a right slot, is ORB_ERR_CAPACITY with nothing leaked); ORB_ERR_ARG also for mb or mbf not
 * finite, when the context's last batch has fewer than 2 * npairs frames or another kp_cap, and for kp_cap above
 * ORB_STEREO_MAX_RIGHT. */
int orb_frames_create_from_batch_stereo(orb_ctx* ctx, const orb_distortion* dist, int npairs, float mb, float mbf,
                                        const uint8_t* d_desc, const orb_keypoint* d_kps_raw, const int* d_counts,
                                        int kp_cap, float min_x, float min_y, float inv_w, float inv_h, float* d_uright,
                                        float* d_depth, orb_frame** out);

/* ======================= Fisheye driver input: mask, crop, half-size and gray (mono_fisheye) ============= */

/* What Examples/Monocular/mono_fisheye.cc:94-116 does to the camera frame before System::TrackMonocularWithBirdview,
 * and the cvtColor Tracking::GrabImageMonocularWithBirdview opens with (Tracking.cc:278-307), as one definition over a
 * source of sw x sh interleaved 8-bit pixels.  `code` is ORB_PREP_GRAY (one byte per pixel: a gray camera) or an
 * ORB_COLOR_* code (3 or 4 bytes per pixel in the order the code names).  The output is the cw/2 x ch/2 GRAY image
 * the reference's extractor receives.  The definition is pinned to OpenCV 3.2 on x86-64 without IPP:
 *   mask    applyMask (:202-212): a source pixel whose mask byte is > 250 has all its channels set to 0.  The mask has
 *           the source's size; the byte is channel 1 of a 3-channel mask (mask.at<Vec3b>(i, j)[1]) or the only channel
 *           of a 1-channel one.  It is read in SOURCE coordinates, before the crop.  mask NULL: nothing is zeroed.
 *   crop    Rect(cx, cy, cw, ch) (:111-113): 0 <= cx, 0 <= cy, cx + cw <= sw, cy + ch <= sh.
 *   resize  cv::resize(im, im, Size(0, 0), 0.5, 0.5) (:116): for an exact factor of 2 INTER_LINEAR takes the INTER_AREA
 *           fast path, per channel D = (S00 + S01 + S10 + S11 + 2) >> 2 over the 2x2 block; every channel on its own; a
 *           masked pixel contributes 0 and is not left out of the mean.
 *   gray    3 or 4 channels: orb_to_gray_host's formula over the three AVERAGED channels (resize, then convert, as
 *           the reference orders them; convert-then-resize differs by one level for some inputs); alpha is ignored.
 *           ORB_PREP_GRAY: the averaged value itself.
 * cw and ch must be EVEN: with an odd side OpenCV leaves the area path for a fractional-scale bilinear resize of the
 * colour image, which is not built (ORB_ERR_ARG).  Scale factors other than 0.5 are not built either.
 * Rows are stride bytes apart; any base alignment and any stride are accepted.  Only the crop rows' [cx * channels,
 * (cx + cw) * channels) bytes are read and only [row, row + cw / 2) of the destination written.
 *   orb_front_prep_host    the definition, on the CPU.  No context, no GPU.
 *   orb_prep_create        one camera's source size, mask (host memory, may be NULL) and crop, resident on ctx's device:
 *                          the mask is reduced once to 4 keep bits per output pixel over the crop.  Synchronous.  Lifetime
 *                          and device rules are orb_rectify's: usable with any context of the same device, one thread at
 *                          a time, destroyed before the context that created it.  cw == 0 or ch == 0 gives an empty
 *                          handle (every call through it is ORB_OK with nothing touched).
 *   orb_prep_size          the output's (cw / 2, ch / 2).
 *   orb_prep_source_size   the source's (sw, sh): the size every frame given with the handle must have.
 *   orb_front_prep_device  nframes source frames in device memory in one launch (k_front_prep), asynchronous on the
 *                          context's stream: frame f at d_src + f * src_frame_pitch -> d_dst + f * dst_frame_pitch.  d_dst
 *                          is what orb_extract_batch_device consumes (same stream: no synchronisation in between).
 *   orb_extract_fisheye    orb_extract for a raw host frame of the handle's source size: only the crop's rows and columns
 *                          are uploaded, prepared on the device, then orb_extract's single-frame chain runs unchanged on
 *                          the prepared image.  orb_get_level(ctx, 0, ...) afterwards returns the prepared gray image.
 *                          Empty image (img == NULL or an empty handle): ORB_OK, the outputs untouched; capacity as
 *                          orb_extract.
 * ORB_ERR_ARG before any GPU work, outputs untouched: an unknown code; mask_channels outside {1, 3} with a mask; a
 * negative size, crop or nframes; an odd cw or ch; a crop outside the source; a source side above 8192 (the output side
 * stays within the extractor's 4096); a source stride below sw * channels, a mask stride below sw * mask_channels, a
 * destination stride below cw / 2; with nframes > 1 a frame pitch below (rows - 1) * stride + the row's bytes; NULL
 * arrays with a non-empty crop; a NULL handle or one of another device than the context's.  nframes == 0: ORB_OK,
 * nothing touched.
 *
 * ConvertMaskBirdview (mono_fisheye.cc:99, :244-271), which the driver runs on the birdview mask of EVERY frame:
 *   dst = (src[1] < 20) ? 0 : 250   over a 3-channel (or 4-channel) mask, then the vehicle footprint zeroed: exactly
 *   orb_bird_footprint_mask's rectangle.  The value is 250, not 255.
 *   orb_bird_mask_host     the definition, on the CPU: the conversion, then orb_bird_footprint_mask.
 *   orb_bird_mask_device   nframes masks in device memory in one launch (k_bird_mask), asynchronous on the context's
 *                          stream.  d_dst with dst_row_stride / dst_frame_pitch is what orb_bird_extract_batch_device
 *                          takes as d_masks with mask_stride / mask_frame_pitch.  The birdview object has a STREAM OF ITS
 *                          OWN: call orb_sync before d_dst goes to orb_bird_extract_device or
 *                          orb_bird_extract_batch_device.
 * ORB_ERR_ARG before any GPU work, outputs untouched: channels outside {3, 4}; a negative size or nframes; a side above
 * 4096; strides below a row; with nframes > 1 a frame pitch below (h - 1) * stride + the row's bytes; NULL arrays with
 * a non-empty mask.  nframes == 0, w == 0 or h == 0: ORB_OK, nothing touched. */
enum { ORB_PREP_GRAY = -1 };   /* a one-channel source, beside the ORB_COLOR_* codes */
typedef struct orb_prep orb_prep;
int  orb_front_prep_host(int code, const uint8_t* src, int sw, int sh, size_t src_stride, const uint8_t* mask,
                         int mask_channels, size_t mask_stride, int cx, int cy, int cw, int ch, uint8_t* dst,
                         size_t dst_stride);
int  orb_prep_create(orb_ctx* ctx, int sw, int sh, const uint8_t* mask, int mask_channels, size_t mask_stride, int cx,
                     int cy, int cw, int ch, orb_prep** out);
void orb_prep_destroy(orb_prep* prep);
int  orb_prep_size(const orb_prep* prep, int* w, int* h);
int  orb_prep_source_size(const orb_prep* prep, int* sw, int* sh);
int  orb_front_prep_device(orb_ctx* ctx, const orb_prep* prep, int code, const uint8_t* d_src, int nframes,
                           size_t src_frame_pitch, size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch,
                           size_t dst_row_stride);
int  orb_extract_fisheye(orb_ctx* ctx, const orb_prep* prep, int code, const uint8_t* img, size_t stride,
                         orb_keypoint* kps, int cap, int* n, uint8_t* desc);
int  orb_bird_mask_host(int channels, const uint8_t* src, int w, int h, size_t src_stride, uint8_t* dst,
                        size_t dst_stride);
int  orb_bird_mask_device(orb_ctx* ctx, int channels, const uint8_t* d_src, int nframes, int w, int h,
                          size_t src_frame_pitch, size_t src_row_stride, uint8_t* d_dst, size_t dst_frame_pitch,
                          size_t dst_row_stride);

/* ======================= DBoW2 vocabulary transform ======================= */

typedef struct orb_vocab orb_vocab;

/* TemplatedVocabulary::loadFromBinaryFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1466-1510)
 * of an ORB vocabulary (ORBvoc.bin format: header nb_nodes, size_node = 41, k, L, scoring,
 * weighting; records parent:int32 | desc[32] | weight:float | isLeaf:u8), onto ctx's device. */
int  orb_vocab_load(orb_ctx* ctx, const char* path, orb_vocab** out);
void orb_vocab_destroy(orb_vocab* v);
int  orb_vocab_info(const orb_vocab* v, int* k, int* L, int* scoring, int* weighting, int* nnodes, int* nwords);

/* Per-feature part of TemplatedVocabulary::transform (:1240-1277): word id, word weight and the node
 * `levelsup` levels above the leaf (FeatureVector key) of each of n descriptors, on the GPU.  Host
 * pointers, synchronous. */
int orb_vocab_transform(orb_ctx* ctx, const orb_vocab* v, const uint8_t* desc, int n, int levelsup, int* word_id,
                        float* weight, uint32_t* node_id);

/* Same for frames 0..nframes-1 of the last orb_extract_batch_device on ctx: outputs at
 * [f * kp_cap + i] (device pointers), counts from that batch.  Asynchronous. */
int orb_vocab_transform_batch_device(orb_ctx* ctx, const orb_vocab* v, int nframes, int levelsup, int* d_word,
                                     float* d_weight, uint32_t* d_node);

/* Host assembly of TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)
 * (:1139-1210) from the per-feature triples, in feature order: BowVector as nbow (word, value)
 * pairs ascending by word; FeatureVector as nfv nodes ascending with CSR fv_off (nfv+1) / fv_idx.
 * Every output array needs room for n entries (fv_off n+1). */
int orb_vocab_bow(const orb_vocab* v, int n, const int* word_id, const float* weight, const uint32_t* node_id,
                  int* bow_words, double* bow_values, int* nbow, uint32_t* fv_nodes, int* fv_off, int* fv_idx,
                  int* nfv);

/* ============ MapPoint::ComputeDistinctiveDescriptors, batched ============ */

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307; MapPointBird.cc:87-152): for each
 * of nmp map points, the descriptors of its observations from non-bad keyframes (observation order)
 * are desc[offsets[m] .. offsets[m+1]) (32 B each); best_idx[m] receives the index (within the point's
 * list) of the descriptor with the least median distance to the others — first on ties — or -1 for
 * an empty list (the reference returns without touching mDescriptor).  Host pointers, synchronous. */
int orb_distinctive_descriptors(orb_ctx* ctx, int nmp, const int* offsets, const uint8_t* desc, int* best_idx);

/* ======================= KeyFrameDatabase: loop and relocalisation candidates ======================= */

/* The step between ComputeBoW and the candidates' SearchByBoW: KeyFrameDatabase (src/KeyFrameDatabase.cc:33-309) and
 * ORBVocabulary::score for an L1 vocabulary (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), with the BowVectors of
 * the live keyframes resident on the context's device.  A BowVector is nbow (word, value) pairs, words strictly
 * ascending and >= 0, values finite (orb_vocab_bow's output).  Every entry point returns ORB_ERR_ARG before any GPU
 * work for a NULL handle or NULL outputs, negative counts, words that are negative or not strictly ascending, a value
 * that is not finite, and a handle of another device than the context's.  One thread at a time per handle; the handle
 * is destroyed before its context.
 * ONLY L1 SCORING is offered (the ORB vocabulary's): L2Scoring sums vi * wi, whose contraction into an FMA the
 * reference build leaves to its compiler flags and which would have to be pinned first.
 *
 *   orb_kfdb_create / destroy   an empty database on ctx's device / frees it.
 *   orb_kfdb_add       KeyFrameDatabase::add (:40-46).  *id = the add sequence number: ids start at 0, count up and are
 *                      never reused.  The pool starts at 1,024 words and grows by doubling.
 *   orb_kfdb_erase     KeyFrameDatabase::erase (:48-67): the entry is flagged, the others keep their order; an unknown
 *                      or already erased id is ORB_ERR_ARG.  Once more than half of the pool is dead the next add or
 *                      query packs it again (order and ids unchanged).
 *   orb_kfdb_clear     KeyFrameDatabase::clear (:69-73); ids keep counting up.
 *   orb_kfdb_size      live entries (0 for NULL).
 *   orb_kfdb_query     the sharing-list loops of DetectLoopCandidates (:86-104) and DetectRelocalizationCandidates
 *                      (:207-222), and the scores of :133 / :249 and of LoopClosing::DetectLoop's minScore loop
 *                      (LoopClosing.cc:122-141), in one launch and one synchronisation.  Returns, in the order of
 *                      lKFsSharingWords (ascending index of the keyframe's first common word within the query, then add
 *                      sequence), every live keyframe that is not in excl_ids and shares at least one word: ids[i],
 *                      common[i] (mnLoopWords / mnRelocWords) and score[i], the DOUBLE L1Scoring::score(query, keyframe)
 *                      returns, byte for byte (terms added in ascending word order, one at a time).  That is a superset
 *                      of the keyframes the reference scores; orb_kfdb_candidates applies the cut.  excl_ids are
 *                      spConnectedKeyFrames (:78, :96); excl_score (nexcl entries, or NULL) receives the same double for
 *                      each excluded keyframe, -0.0 when it shares no word; an excluded id that was erased is accepted
 *                      and ignored and its excl_score left untouched; an id that was never issued is ORB_ERR_ARG.
 *                      ORB_ERR_CAPACITY with *n set when cap < *n; every output array is then untouched.  nbow == 0 or
 *                      an empty database: ORB_OK, *n = 0, no GPU work.
 *   orb_kfdb_candidates  pure host: everything after the sharing list, for either form (:107-196 LOOP, :224-308 RELOC),
 *                      on orb_kfdb_query's outputs: int minCommonWords = maxCommonWords * 0.8f, float si = score, the
 *                      covisibility accumulation in float over nb(user, id, out, 10) = GetBestCovisibilityKeyFrames(10)
 *                      (the callback writes up to cap ids in the reference's order and returns their number; it is called
 *                      only for the entries of lScoreAndMatch, in order), 0.75f * bestAccScore, first occurrence of
 *                      each best keyframe.  cand_ids needs room for n ids.  RELOC: a neighbour counts iff it is in the
 *                      list, scored or not, and contributes its mRelocScore, which lives in the handle, is set by every
 *                      RELOC call that scores the keyframe, and is 0.0f until then (PINNED: the reference leaves it
 *                      uninitialised, KeyFrame.cc:35); min_score is ignored.  LOOP: lScoreAndMatch holds si >= min_score,
 *                      a neighbour counts iff it is in the list and above the cut, with this call's score;
 *                      bestAccScore starts at min_score.  db == NULL is accepted by this entry point alone: a call
 *                      without state (every mRelocScore reads 0.0f before this call scores it; nothing is kept).
 *   orb_bow_score      pure host: ORBVocabulary::score(v1, v2) of an L1 vocabulary.
 *   orb_kfdb_query_lds_words  the longest query orb_kfdb_query stages in LDS; a longer one is read from global memory
 *                      (same results). */
typedef struct orb_kfdb orb_kfdb;
int  orb_kfdb_create(orb_ctx* ctx, orb_kfdb** out);
void orb_kfdb_destroy(orb_kfdb* db);
int  orb_kfdb_add(orb_ctx* ctx, orb_kfdb* db, int nbow, const int* words, const double* values, int* id);
int  orb_kfdb_erase(orb_kfdb* db, int id);
int  orb_kfdb_clear(orb_kfdb* db);
int  orb_kfdb_size(const orb_kfdb* db);
int  orb_kfdb_query(orb_ctx* ctx, orb_kfdb* db, int nbow, const int* words, const double* values,
                    int nexcl, const int* excl_ids, double* excl_score,
                    int cap, int* ids, int* common, double* score, int* n);
typedef int (*orb_kfdb_neighbours_fn)(void* user, int id, int* out, int cap);
enum { ORB_KFDB_RELOC = 0, ORB_KFDB_LOOP = 1 };
int  orb_kfdb_candidates(orb_kfdb* db, int mode, float min_score, int n, const int* ids, const int* common,
                         const double* score, orb_kfdb_neighbours_fn nb, void* user, int* cand_ids, int* ncand);
int  orb_bow_score(int n1, const int* w1, const double* v1, int n2, const int* w2, const double* v2, double* score);
int  orb_kfdb_query_lds_words(void);

#ifdef __cplusplus
}
#endif
#endif
