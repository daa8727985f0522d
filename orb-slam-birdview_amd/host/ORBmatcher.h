/*
 * ORB_SLAM2::ORBmatcher — C++ mirror of the reference's descriptor matchers
 * (include/ORBmatcher.h:37-119, src/ORBmatcher.cc) over liborbgpu's C-ABI.
 *
 * The reference methods take Frame& / KeyFrame* and read a handful of their members; the mirror
 * takes a FeatureSet naming exactly those members (INTEGRATION.md shows the two-line adapter from a
 * Frame / KeyFrame).  Results keep the reference's meaning, with MapPoint* replaced by the index of
 * the feature that owns it:
 *   SearchByBoW(KF, F, v)     v[iF]  = KF feature whose MapPoint the reference assigns, or -1
 *   SearchByBoW(KF1, KF2, v)  v[i1]  = KF2 feature whose MapPoint the reference assigns, or -1
 * Distances and candidate filtering run on the GPU; the order-dependent acceptance (taken sets,
 * vMatchedDistance, rotation histogram) is replayed in the reference's iteration order, so match
 * indices are identical to the reference's.  GPU failures throw ORB_SLAM2::OrbGpuError.
 */
#ifndef ORBGPU_HOST_ORBMATCHER_H
#define ORBGPU_HOST_ORBMATCHER_H

#include <map>
#include <utility>
#include <vector>

#include "ORBextractor.h"

// The matcher lives in ORB_SLAM2 like the reference's.  When integrated next to the reference's own
// ORB_SLAM2::ORBmatcher (which keeps the pose arithmetic of the projection searches), build with
// -DORBGPU_MATCHER_NAMESPACE=orbgpu_host.
#ifndef ORBGPU_MATCHER_NAMESPACE
#define ORBGPU_MATCHER_NAMESPACE ORB_SLAM2
#endif

namespace ORBGPU_MATCHER_NAMESPACE {

using ORB_SLAM2::DescriptorMat;
using ORB_SLAM2::KeyPoint;
using ORB_SLAM2::OrbGpuError;
using ORB_SLAM2::Point2f;

// DBoW2::FeatureVector (Thirdparty/DBoW2/DBoW2/FeatureVector.h: std::map<NodeId, std::vector<unsigned int>>)
typedef std::map<unsigned int, std::vector<unsigned int> > FeatureVector;

#define ORBGPU_FRAME_GRID_ROWS 48   // Frame.h:39
#define ORBGPU_FRAME_GRID_COLS 64   // Frame.h:40

// Frame::mGrid + GetFeaturesInArea (Frame.cc:378-412, 494-560).  The birdview grid
// (Frame.cc:877-940) is the same structure with minX = minY = 0 and its own cell sizes.
class FrameGrid {
public:
    FrameGrid() = default;
    // Frame grid: cells of (maxX-minX)/64 x (maxY-minY)/48 over mvKeysUn
    FrameGrid(const KeyPoint* keysUn, int n, float minX, float maxX, float minY, float maxY);
    // birdview grid: GridElementWidthInv/HeightInv given directly, origin (0, 0)
    static FrameGrid Birdview(const KeyPoint* keysBird, int n, float widthInv, float heightInv);
    std::vector<size_t> GetFeaturesInArea(float x, float y, float r, int minLevel = -1, int maxLevel = -1) const;
    // the grid as the C-ABI's orb_frame_grid (cells column-major, a cell's keypoints in its vector's order); off and
    // idx receive the CSR arrays the returned struct points into
    orb_frame_grid Csr(std::vector<int>& off, std::vector<int>& idx) const;

private:
    void assign(const KeyPoint* keys, int n);
    const KeyPoint* keys_ = nullptr;
    float minX_ = 0, minY_ = 0, invW_ = 0, invH_ = 0;
    std::vector<std::vector<size_t> > cells_;   // [ix * ROWS + iy]
};

// Frame::UndistortKeyPoints (Frame.cc:571-603) on the GPU: mvKeysUn from mvKeys, mK's entries and mDistCoef's four
// floats (cv::fisheye::undistortPoints as the reference calls it; distCoef[0] == 0 returns the keypoints unchanged).
// The bytes are those of the library's CPU definition, orb_undistort_points_host.  Runs on the calling thread's
// matcher context; failures throw OrbGpuError.
std::vector<KeyPoint> UndistortKeyPoints(float fx, float fy, float cx, float cy, const float distCoef[4],
                                         const std::vector<KeyPoint>& keys);
// Frame::ComputeImageBounds (Frame.cc:605-660): mnMinX, mnMaxX, mnMinY, mnMaxY of a cols x rows image (CPU)
void ComputeImageBounds(float fx, float fy, float cx, float cy, const float distCoef[4], int cols, int rows, float& minX,
                        float& maxX, float& minY, float& maxY);

// A Frame's or KeyFrame's train side kept on the device (the C-ABI's orb_frame): descriptors, undistorted keypoints
// and optionally mvuRight are uploaded once and the library builds the grid on the GPU, so a frame that is searched
// several times is not staged again.  Constructed like a FrameGrid, plus the arrays the searches read; the arrays
// may be freed once the constructor returns.  Move-only; the destructor frees the device memory.  Failures throw
// OrbGpuError.  It lives on the GPU of the calling thread's matcher context (ORBGPU_DEVICE, default 0) and serves any
// thread's searches on that GPU; create it in the Frame / KeyFrame constructor and let it die with its owner
// (INTEGRATION.md).
class ResidentFrame {
public:
    ResidentFrame() = default;
    // Frame grid: cells of (maxX-minX)/64 x (maxY-minY)/48 over mvKeysUn; uRight may be NULL (monocular)
    ResidentFrame(const KeyPoint* keysUn, int n, const uint8_t* descriptors, const float* uRight, float minX, float maxX,
                  float minY, float maxY);
    // birdview grid: GridElementWidthInv/HeightInv given directly, origin (0, 0), no uRight
    static ResidentFrame Birdview(const KeyPoint* keysBird, int n, const uint8_t* descriptors, float widthInv,
                                  float heightInv);
    // from arrays already in the memory of ctx's GPU (e.g. a slot of orb_extract_batch_device's outputs)
    static ResidentFrame FromDevice(orb_ctx* ctx, int n, const uint8_t* d_descriptors, const KeyPoint* d_keysUn,
                                    const float* d_uRight, float minX, float minY, float widthInv, float heightInv);
    // from a slot of orb_extract_batch_device's outputs as the extractor wrote it: n descriptors and RAW keypoints.
    // The library undistorts them on the GPU (Frame::UndistortKeyPoints) and builds the grid from the undistorted
    // ones; the bounds are ComputeImageBounds'.  k[0] == 0 is the reference's identity path.
    static ResidentFrame FromExtraction(orb_ctx* ctx, const orb_distortion& dist, int n, const uint8_t* d_descriptors,
                                        const KeyPoint* d_keysRaw, const float* d_uRight, float minX, float maxX,
                                        float minY, float maxY);
    // the same for all nframes slots of a batch (frame f's arrays at f * kp_cap, its count in d_counts[f]): one
    // undistort launch for the whole batch
    static std::vector<ResidentFrame> FromBatch(orb_ctx* ctx, const orb_distortion& dist, int nframes,
                                                const uint8_t* d_descriptors, const KeyPoint* d_keysRaw,
                                                const int* d_counts, int kp_cap, float minX, float maxX, float minY,
                                                float maxY);
    // the RGB-D Frame constructor after extraction (Frame.cc:145-200) for a batch: FromBatch, with
    // Frame::ComputeStereoFromRGBD run on the undistorted keypoints between the undistort step and the grids.  depth:
    // the batch's depth maps in device memory (include/orbgpu.h orb_depth_map).  d_uRight / d_depth (nframes * kp_cap
    // floats each, device memory, either may be NULL) receive mvuRight / mvDepth; every frame carries its uRight.
    static std::vector<ResidentFrame> FromBatchRGBD(orb_ctx* ctx, const orb_distortion& dist, const orb_depth_map& depth,
                                                    float mbf, int nframes, const uint8_t* d_descriptors,
                                                    const KeyPoint* d_keysRaw, const int* d_counts, int kp_cap,
                                                    float minX, float maxX, float minY, float maxY, float* d_uRight,
                                                    float* d_depth);
    // the stereo Frame constructor after extraction (Frame.cc:129-141) for a batch of 2 * npairs frames extracted on
    // ctx (slots 2p, 2p + 1 = left, right): UndistortKeyPoints of the left keypoints, Frame::ComputeStereoMatches on
    // the raw ones, the left frames' grids (orb_frames_create_from_batch_stereo).  d_uRight / d_depth (npairs * kp_cap
    // floats each, device memory, either may be NULL) receive mvuRight / mvDepth; every frame carries its uRight.
    static std::vector<ResidentFrame> FromBatchStereo(orb_ctx* ctx, const orb_distortion& dist, int npairs, float mb,
                                                      float mbf, const uint8_t* d_descriptors, const KeyPoint* d_keysRaw,
                                                      const int* d_counts, int kp_cap, float minX, float maxX,
                                                      float minY, float maxY, float* d_uRight, float* d_depth);
    ~ResidentFrame();
    ResidentFrame(ResidentFrame&& o) noexcept;
    ResidentFrame& operator=(ResidentFrame&& o) noexcept;
    ResidentFrame(const ResidentFrame&) = delete;
    ResidentFrame& operator=(const ResidentFrame&) = delete;

    int N() const { return n_; }
    bool hasURight() const { return hasURight_; }
    explicit operator bool() const { return h_ != nullptr; }
    const orb_frame* handle() const { return h_; }
    // the grid the GPU built, as FrameGrid::Csr gives the host one (cell_off: 64 * 48 + 1 entries)
    void Grid(std::vector<int>& off, std::vector<int>& idx) const;

    // BoW on the handle (orb_frame_compute_bow): Frame::ComputeBoW / KeyFrame::ComputeBoW over the resident
    // descriptors, the FeatureVector built on the GPU.  ctx / vocab: ORBVocabulary::context() / handle().  The static
    // form serves several frames with one pair of launches.  SetFeatVec attaches an mFeatVec the caller holds; BoW
    // reads both vectors back (an empty BowVector after SetFeatVec).  The handle then serves the ResidentFrame
    // overloads of ORBmatcher::SearchByBoW / SearchForTriangulation.
    void ComputeBoW(orb_ctx* ctx, const orb_vocab* vocab, int levelsup = 4);
    static void ComputeBoW(orb_ctx* ctx, const orb_vocab* vocab, const std::vector<ResidentFrame*>& frames,
                           int levelsup = 4);
    void SetFeatVec(const FeatureVector& featVec);
    void BoW(const orb_vocab* vocab, std::map<unsigned int, double>& bowVec, FeatureVector& featVec) const;
    bool hasBoW() const { return orb_frame_has_bow(h_) != 0; }

private:
    orb_frame* h_ = nullptr;
    int n_ = 0;
    bool hasURight_ = false;
    size_t fvCap_ = 0;   // the entries of a FeatureVector given by SetFeatVec (BoW sizes its arrays by it)
};

// Map points kept on the device (the C-ABI's orb_points): per slot GetWorldPos, GetNormal, the raw mfMinDistance /
// mfMaxDistance and GetDescriptor.  Write() fills or rewrites a slot range and grows the handle; a point whose
// position, normal, distances or descriptor changed is written again.  ORBmatcher::SearchLocalPoints and
// FuseSearch(const ResidentPoints&, ...) project and search the slots without staging them.  Move-only; the destructor
// frees the device memory; failures throw OrbGpuError.  It lives on the GPU of the calling thread's matcher context,
// like a ResidentFrame.
class ResidentPoints {
public:
    ResidentPoints() = default;
    explicit ResidentPoints(int capacity);
    ~ResidentPoints();
    ResidentPoints(ResidentPoints&& o) noexcept;
    ResidentPoints& operator=(ResidentPoints&& o) noexcept;
    ResidentPoints(const ResidentPoints&) = delete;
    ResidentPoints& operator=(const ResidentPoints&) = delete;

    // slots first .. first + n - 1: pos and normal 3 n floats, the distances n floats, descriptors 32 n bytes
    void Write(int first, int n, const float* pos, const float* normal, const float* minDistance,
               const float* maxDistance, const uint8_t* descriptors);
    int Capacity() const { return orb_points_capacity(h_); }
    explicit operator bool() const { return h_ != nullptr; }
    const orb_points* handle() const { return h_; }

private:
    orb_points* h_ = nullptr;
};

// One target keyframe of FuseSearch(const ResidentPoints&, ...): Fuse(pKF, vpMapPoints, th) with the points as slots
struct FusePointsTarget {
    orb_camera camera;                        // pKF's pose and intrinsics (orbgpu.h)
    const ResidentFrame* kf = nullptr;        // pKF
    const float* invLevelSigma2 = nullptr;    // pKF->mvInvLevelSigma2, camera.nlevels entries
    float th = 3.0f;
    std::vector<int> ids;                     // the slots of the points that are neither bad nor IsInKeyFrame(pKF)
};

// The members of a Frame / KeyFrame that ORBmatcher reads, as zero-copy views (cv::KeyPoint and
// orb_keypoint share one 28-byte layout; a continuous n x 32 CV_8U Mat is n*32 bytes).  Pointers
// may be NULL where a method does not read the member (see each method).
struct FeatureSet {
    int n = 0;                                        // N (Frame::N / KeyFrame::N / mvKeysBird.size())
    const KeyPoint* keys = nullptr;                   // Frame::mvKeys / KeyFrame::mvKeysUn / mvKeysBird
    const uint8_t* descriptors = nullptr;             // mDescriptors / mDescriptorsBird, row-major n x 32
    const FeatureVector* featVec = nullptr;           // mFeatVec
    const uint8_t* hasMapPoint = nullptr;             // per feature: MapPoint != NULL (&& !isBad() where read)
    const float* uRight = nullptr;                    // mvuRight
    const float* scaleFactors = nullptr;              // mvScaleFactors
    const float* levelSigma2 = nullptr;               // mvLevelSigma2
    int nlevels = 0;                                  // mnScaleLevels (length of the two tables above)
    const FrameGrid* grid = nullptr;                  // mGrid / mGridBirdview
    const float* invLevelSigma2 = nullptr;            // mvInvLevelSigma2 (Fuse's reprojection gate)
    // The frame as a ResidentFrame: where a search reads grid, descriptors and uRight of its TRAIN side (the
    // projection searches' Frame, the window matches' F2, SearchByMatchBird's Frame / CurrentFrame... see below), it
    // takes them from the handle instead and does not read those three members; n must equal resident->N().  The
    // other members (hasMapPoint, the scale tables, keys where a method reads them on the host) are read as before.
    const ResidentFrame* resident = nullptr;
    int N() const { return n; }
};
// Tags standing for the reference's Frame& and KeyFrame* arguments (so the overloads keep the
// reference's names: SearchByBoW(KeyFrame*, Frame&) vs SearchByBoW(KeyFrame*, KeyFrame*)).
struct FrameData : FeatureSet {};
struct KeyFrameData : FeatureSet {};

// What the projection-gated searches read of each projected map point: values the caller already holds
// (Frame::isInFrustum stores them in the MapPoint; TrackWithMotionModel computes them in its loop).  The points the
// reference skips before its search are left out by the caller (each struct says which), as SearchForTriangulation's
// epipole is computed by the caller.  A result vector holds, per Frame feature, the index (into `points`) of the
// map point the reference assigns to it, -1 where it assigns none, -2 where the rotation cull reset it to NULL.
struct ProjectedLastFrame {   // SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
    struct Point {            // LastFrame feature i with a MapPoint, !mvbOutlier[i], invzc >= 0, (u, v) inside the
        float u, v;           //   CurrentFrame's bounds (ORBmatcher.cc:1355-1376): the projection (:1370-1371)
        float invzc;          // 1 / x3Dc.z (:1365)
        int octave;           // LastFrame.mvKeys[i].octave (:1378)
        float angle;          // LastFrame.mvKeysUn[i].angle (:1433)
        bool observed;        // pMP->Observations() > 0 (false: a temporal point of Tracking::UpdateLastFrame)
        const uint8_t* descriptor;   // pMP->GetDescriptor(), 32 bytes
    };
    std::vector<Point> points;
    bool bForward = false, bBackward = false;   // :1348-1349 (ignored when bMono)
    float mbf = 0;                              // CurrentFrame.mbf
};
struct ProjectedMapPoints {   // SearchByProjection(Frame& F, const vector<MapPoint*>&, th)
    struct Point {            // a MapPoint with mbTrackInView && !isBad() (:54-58)
        float projX, projY, projXR;   // mTrackProjX, mTrackProjY, mTrackProjXR
        int level;                    // mnTrackScaleLevel
        float viewCos;                // mTrackViewCos
        const uint8_t* descriptor;
    };
    std::vector<Point> points;
};
struct ProjectedBirdPoints {   // SearchByProjectionBird(Frame& F, const vector<MapPointBird*>&, r)
    struct Point {             // mnLastFrameSeen != F.mnId, |localPos.z| <= 0.2, pt inside the birdview (:1933-1943)
        float x, y;            // Frame::ProjectXYZ2Birdview(localPos) (:1940)
        const uint8_t* descriptor;
    };
    std::vector<Point> points;
};

struct KeyFrameBirdPoints {    // SearchByMatchBird(KeyFrame* pKF, Frame& F, vector<MapPointBird*>&, r)
    struct Point {             // a birdview keypoint k of pKF with GetMapPointMatchesBird()[k] != NULL (:2016-2018)
        int index;             // k: what the result vector holds for the Frame feature this point is matched to
        float x, y, angle;     // pKF->mvKeysBird[k].pt and .angle (:2020-2021, :2079)
        const uint8_t* descriptor;   // pMPBird->GetDescriptor(), 32 bytes
    };
    std::vector<Point> points; // in ascending k, the order of the reference's loop
};

// The keyframe searches (Fuse, SearchBySim3, the keyframe forms of SearchByProjection).  The caller keeps the pose
// arithmetic (Rcw*p3Dw+tcw, IsInImage, the distance and viewing-angle tests, PredictScale), leaves out the points the
// reference skips before its search, and keeps each point's index.
struct ProjectedKFPoint {
    float u, v, ur;              // the projection; ur = u - bf*invz (read by Fuse's reprojection gate only)
    int predictedLevel;          // pMP->PredictScale(dist3D, pKF)
    float radius;                // th * pKF->mvScaleFactors[predictedLevel]
    const uint8_t* descriptor;   // pMP->GetDescriptor(), 32 bytes
};
struct FuseTarget {              // one Fuse call: a target keyframe and the map points projected into it
    KeyFrameData kf;             // keys (mvKeysUn), descriptors, grid; uRight and invLevelSigma2 with the chi2 gate
    std::vector<ProjectedKFPoint> points;
};
struct FuseBest {                // bestIdx / bestDist of ORBmatcher.cc:901-949, before `bestDist<=TH_LOW`; -1 / -1: none
    int idx, dist;
};
struct ProjectedSim3Points {     // SearchBySim3: one keyframe's map points projected into the other (:1150-1189),
    std::vector<int> index;      //   without vbAlreadyMatched ones; index[k] = the point's feature in its own keyframe
    std::vector<ProjectedKFPoint> points;
};
struct ProjectedLoopPoints {     // SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th): the points left after
    std::vector<ProjectedKFPoint> points;   // :317-355
};
struct ProjectedKeyFramePoints { // SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist): pKF's map points
    std::vector<ProjectedKFPoint> points;   // left after :1492-1521 ...
    std::vector<float> angle;               // ... and pKF->mvKeysUn[i].angle of each
};

class ORBmatcher {
public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true);

    // Computes the Hamming distance between two ORB descriptors (ORBmatcher.cc:1647-1663)
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b);

    // ORBmatcher.cc:159-288.  KF: keys (mvKeysUn), descriptors, featVec, hasMapPoint (MP && !isBad);
    // F: keys (mvKeys), descriptors, featVec.
    int SearchByBoW(const KeyFrameData& KF, const FrameData& F, std::vector<int>& vpMapPointMatches);
    // ORBmatcher.cc:522-655.  Both: keys (mvKeysUn), descriptors, featVec, hasMapPoint (MP && !isBad).
    int SearchByBoW(const KeyFrameData& KF1, const KeyFrameData& KF2, std::vector<int>& vpMatches12);

    // ORBmatcher.cc:405-520.  F1: keys (mvKeysUn), descriptors; F2: keys, descriptors, grid.
    int SearchForInitialization(const FrameData& F1, const FrameData& F2, std::vector<Point2f>& vbPrevMatched,
                                std::vector<int>& vnMatches12, int windowSize = 10);

    // ORBmatcher.cc:657-823.  Both: keys (mvKeysUn), descriptors, featVec, hasMapPoint (GetMapPoint != NULL),
    // uRight; KF2: scaleFactors, levelSigma2.  F12 row-major 3x3; (ex, ey) = epipole of KF1's camera
    // centre in KF2 (:662-668, computed by the caller from the poses).
    int SearchForTriangulation(const KeyFrameData& KF1, const KeyFrameData& KF2, const float F12[9], float ex, float ey,
                               std::vector<std::pair<size_t, size_t> >& vMatchedPairs, const bool bOnlyStereo);
    // KF1 against several KF2s in one call (LocalMapping.cc:247-278's neighbour loop; orb_search_for_triangulation_batch):
    // vvMatchedPairs[p] == SearchForTriangulation(KF1, *neighbours[p].KF2, ...) for the same inputs.  Returns the total.
    struct TriangulationNeighbour {
        const KeyFrameData* KF2;
        float F12[9];
        float ex, ey;
    };
    int SearchForTriangulation(const KeyFrameData& KF1, const std::vector<TriangulationNeighbour>& neighbours,
                               std::vector<std::vector<std::pair<size_t, size_t> > >& vvMatchedPairs, const bool bOnlyStereo);

    // The three vocabulary-gated searches between ResidentFrames that carry BoW (ComputeBoW / SetFeatVec; the
    // triangulation also needs uRight on both): results equal the KeyFrameData forms' on the same members, and only
    // the map-point flags (one byte per feature, n entries each) go up per call.  The KeyFrameData forms above do not
    // route here.
    int SearchByBoW(const ResidentFrame& KF, const uint8_t* hasMapPointKF, const ResidentFrame& F,
                    std::vector<int>& vpMapPointMatches);
    int SearchByBoW(const ResidentFrame& KF1, const uint8_t* hasMapPoint1, const ResidentFrame& KF2,
                    const uint8_t* hasMapPoint2, std::vector<int>& vpMatches12);
    struct ResidentTriangulationNeighbour {
        const ResidentFrame* KF2;
        const uint8_t* hasMapPoint;     // GetMapPoint(i) != NULL, KF2->N() entries
        const float* scaleFactors;      // pKF2->mvScaleFactors
        const float* levelSigma2;       // pKF2->mvLevelSigma2
        int nlevels;
        float F12[9];
        float ex, ey;
    };
    int SearchForTriangulation(const ResidentFrame& KF1, const uint8_t* hasMapPoint1,
                               const std::vector<ResidentTriangulationNeighbour>& neighbours,
                               std::vector<std::vector<std::pair<size_t, size_t> > >& vvMatchedPairs,
                               const bool bOnlyStereo);

    // ORBmatcher.cc:1667-1789 (window around vPrevMatched, level-0 only, updates vPrevMatched) and
    // :1790-1899 (window around each keypoint).  F1: keys (mvKeysBird), descriptors;
    // F2: keys, descriptors, grid (FrameGrid::Birdview).
    int BirdviewMatch(const FrameData& F1, const FrameData& F2, std::vector<int>& vnMatches12,
                      std::vector<Point2f>& vPrevMatched, int windowSize = 10);
    int BirdviewMatch(const FrameData& F1, const FrameData& F2, std::vector<int>& vnMatches12, int windowSize = 10);

    // Every method that takes a FrameGrid plus arrays as its train side also accepts that side as a ResidentFrame:
    // set FeatureSet::resident (or use the overloads below, which do so) and the call goes to the handle form of the
    // C-ABI with results equal to the FrameGrid form's.  That covers SearchForInitialization / BirdviewMatch (F2;
    // F2.keys are still read on the host to update vbPrevMatched), the three Frame forms and the two keyframe forms of
    // SearchByProjection, SearchByProjectionBird, SearchByMatchBird(KF, F), FuseSearch and SearchBySim3 (each
    // target's kf).  SearchByMatchBird(CurrentFrame, LastFrame) has no handle form in the C-ABI and ignores it.
    int SearchByProjection(const ResidentFrame& CurrentFrame, FrameData& members, const ProjectedLastFrame& LastFrame,
                           const float th, const bool bMono, std::vector<int>& vpMapPointMatches);
    int SearchByProjection(const ResidentFrame& F, FrameData& members, const ProjectedMapPoints& vpMapPoints,
                           const float th, std::vector<int>& vpMapPointMatches);
    int SearchByProjectionBird(const ResidentFrame& F, FrameData& members, const ProjectedBirdPoints& vpMapPointsBird,
                               const float r, std::vector<int>& vpMapPointMatchesBird);
    int SearchByMatchBird(const KeyFrameBirdPoints& KF, const ResidentFrame& F, std::vector<int>& vpMapPointMatchesBird,
                          const float r);
    int BirdviewMatch(const FrameData& F1, const ResidentFrame& F2, std::vector<int>& vnMatches12, int windowSize = 10);

    // ORBmatcher.cc:1328-1470.  CurrentFrame: keys (mvKeysUn), descriptors, grid, uRight (NULL: monocular, all -1),
    // hasMapPoint (mvpMapPoints[i] && Observations() > 0; NULL: none), scaleFactors, nlevels.
    int SearchByProjection(FrameData& CurrentFrame, const ProjectedLastFrame& LastFrame, const float th, const bool bMono,
                           std::vector<int>& vpMapPointMatches);
    // ORBmatcher.cc:45-129.  F: as above.
    int SearchByProjection(FrameData& F, const ProjectedMapPoints& vpMapPoints, const float th,
                           std::vector<int>& vpMapPointMatches);
    // ORBmatcher.cc:1923-1998.  F: keys (mvKeysBird), descriptors (mDescriptorsBird), grid (FrameGrid::Birdview),
    // hasMapPoint (mvpMapPointsBird[i] && Observations() > 0).
    int SearchByProjectionBird(FrameData& F, const ProjectedBirdPoints& vpMapPointsBird, const float r,
                               std::vector<int>& vpMapPointMatchesBird);

    // ORBmatcher.cc:2000-2114.  F: keys (mvKeysBird), descriptors (mDescriptorsBird), grid (FrameGrid::Birdview).
    // vpMapPointMatchesBird (sized to F.N()): per Frame feature the `index` of the keyframe point whose MapPointBird
    // the reference leaves there, -1 = none, -2 = reset to NULL by the rotation cull.  The return value is the
    // reference's nmatches (steals count twice, culled double entries are taken off twice).  TrackReferenceKeyFrame's
    // retry with the larger radius (Tracking.cc:1046 / :1049) is a second call.
    int SearchByMatchBird(const KeyFrameBirdPoints& KF, FrameData& F, std::vector<int>& vpMapPointMatchesBird,
                          const float r);
    // ORBmatcher.cc:1901-1921.  LastFrame: keys (mvKeysBird), descriptors, hasMapPoint (mvpMapPointsBird[k] != NULL;
    // NULL: none); CurrentFrame: keys, descriptors, grid (FrameGrid::Birdview).  vpMapPointsBird (sized to
    // CurrentFrame.N()): per CurrentFrame feature the LastFrame feature whose MapPointBird the reference writes into
    // CurrentFrame.mvpMapPointsBird there, -1 where it leaves the slot as it is.  Returns the points carried over.
    int SearchByMatchBird(FrameData& CurrentFrame, const FrameData& LastFrame, const int windowSize,
                          std::vector<int>& vpMapPointsBird);

    // The inner searches of Fuse for many target keyframes in one GPU call: chi2Gate = true is Fuse(KeyFrame*, const
    // vector<MapPoint*>&, th) (ORBmatcher.cc:823-975, LocalMapping::SearchInNeighbors), false is Fuse(KeyFrame*, Scw,
    // ...) (:977-1100, LoopClosing::SearchAndFuse).  best[t][i] belongs to targets[t].points[i]; what follows the
    // search (:952-971) is the caller's replay.
    void FuseSearch(const std::vector<FuseTarget>& targets, bool chi2Gate, std::vector<std::vector<FuseBest> >& best);
    // The same search (chi2 gate) with the projection on the GPU too: target t's points are the slots targets[t].ids
    // of `points`, projected through targets[t].camera as ORBmatcher.cc:852-890 does; best[t][i] belongs to ids[i],
    // -1 / -1 for a point the projection rejects.  proj (optional) receives the records (orb_point_proj).
    void FuseSearch(const ResidentPoints& points, const std::vector<FusePointsTarget>& targets,
                    std::vector<std::vector<FuseBest> >& best,
                    std::vector<std::vector<orb_point_proj> >* proj = nullptr);
    // Tracking::SearchLocalPoints' second loop (Tracking.cc:1635-1660): Frame::isInFrustum(pMP, viewingCosLimit) for
    // the slots ids of `points` through camera, then SearchByProjection(F, vpMapPoints, th) over the visible ones, in
    // one GPU call.  members: hasMapPoint (mvpMapPoints[i] && Observations() > 0; NULL: none).  F's uRight gates if it
    // has one.  vpMapPointMatches (sized to F.N()): per Frame feature the position in ids of the point assigned to it,
    // -1 = none.  proj (optional) receives the records: verdict 0 is isInFrustum returning true.
    int SearchLocalPoints(const ResidentPoints& points, const orb_camera& camera, const std::vector<int>& ids,
                          const ResidentFrame& F, const FrameData& members, const float th,
                          const float viewingCosLimit, std::vector<int>& vpMapPointMatches,
                          std::vector<orb_point_proj>* proj = nullptr);
    // One point of one target on the CPU with another descriptor: a point whose descriptor changed during the replay.
    FuseBest FuseSearchOne(const FuseTarget& target, int point, const uint8_t* descriptor, bool chi2Gate);
    // ORBmatcher.cc:1102-1326: both directions in one GPU call, TH_HIGH and the agreement loop.  vnMatch12[i1] = the
    // KF2 feature both directions agree on, else -1; returns nFound.
    int SearchBySim3(const KeyFrameData& KF1, const KeyFrameData& KF2, const ProjectedSim3Points& points1in2,
                     const ProjectedSim3Points& points2in1, std::vector<int>& vnMatch12);
    // ORBmatcher.cc:290-403.  vpMatched: in, per feature != -1 <=> vpMatched[idx] != NULL; out, the features the call
    // matched hold the index of their point.  Returns nmatches.
    // The radius is th * KF.scaleFactors[predictedLevel] (:360; the points' own radius is not read).
    int SearchByProjection(KeyFrameData& KF, const ProjectedLoopPoints& vpPoints, const int th,
                           std::vector<int>& vpMatched);
    // ORBmatcher.cc:1472-1599.  CurrentFrame.hasMapPoint[i2] = mvpMapPoints[i2] != NULL; the result as for the other
    // Frame forms (-2: reset by the rotation cull).
    int SearchByProjection(FrameData& CurrentFrame, const ProjectedKeyFramePoints& vpPoints, const float th,
                           const int ORBdist, std::vector<int>& vpMapPointMatches);

    static const int TH_LOW;
    static const int TH_HIGH;
    static const int HISTO_LENGTH;

protected:
    int projection_search(int mode, const FeatureSet& F, bool stereo, const std::vector<orb_proj_query>& q,
                          const std::vector<uint8_t>& qdesc, std::vector<int>& matches, const char* what,
                          int max_dist = -1 /* TH_HIGH */, int check_ori = -1 /* mbCheckOrientation */,
                          const uint8_t* taken = nullptr /* F.hasMapPoint */);
    int window_match(bool level0_only, const FeatureSet& F1, const FeatureSet& F2, const std::vector<Point2f>* centres,
                     int windowSize, std::vector<int>& vnMatches12);
    float mfNNratio;
    bool mbCheckOrientation;
};

// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307), batched over map points:
// observations[m] = the descriptors (32 B each, observation order, bad keyframes skipped) of map
// point m.  Returns per point the index of the descriptor the reference copies into mDescriptor, or
// -1 for an empty list (the reference then leaves mDescriptor untouched).
std::vector<int> ComputeDistinctiveDescriptors(const std::vector<std::vector<const uint8_t*> >& observations);

}  // namespace ORBGPU_MATCHER_NAMESPACE

#endif
