// ORB_SLAM2::ORBmatcher over liborbgpu (see ORBmatcher.h).  Marshals the Frame/KeyFrame members
// into the C-ABI's flat arrays; all descriptor distances are computed by the gfx950 kernels.
#include "ORBmatcher.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace ORBGPU_MATCHER_NAMESPACE {

const int ORBmatcher::TH_HIGH = 100;   // ORBmatcher.cc:37-39
const int ORBmatcher::TH_LOW = 50;
const int ORBmatcher::HISTO_LENGTH = 30;

namespace {

void check(int st, const char* what) {
    if (st != ORB_OK) throw OrbGpuError(st, what);
}

// Matchers are stack objects in the reference (one per call site, any thread): they share one
// context per (host thread, device), created on first use.
struct ThreadCtx {
    int device = -1;
    orb_ctx* ctx = nullptr;
    ~ThreadCtx() {
        if (ctx) orb_destroy(ctx);
    }
};

orb_ctx* matcher_ctx() {
    static thread_local ThreadCtx tc;
    const char* e = getenv("ORBGPU_DEVICE");
    const int dev = e ? atoi(e) : 0;
    if (tc.ctx && tc.device == dev) return tc.ctx;
    if (tc.ctx) orb_destroy(tc.ctx);
    tc.ctx = nullptr;
    orb_params p;
    memset(&p, 0, sizeof p);
    p.nfeatures = 1000;
    p.scaleFactor = 1.2f;
    p.nlevels = 8;
    p.iniThFAST = 20;
    p.minThFAST = 7;
    p.device = dev;
    int st = ORB_OK;
    tc.ctx = orb_create(&p, &st);
    if (!tc.ctx) throw OrbGpuError(st, "orb_create (matcher)");
    tc.device = dev;
    return tc.ctx;
}

// DBoW2::FeatureVector -> CSR over ascending node ids (std::map order = the reference's iteration order)
struct Csr {
    std::vector<uint32_t> ids;
    std::vector<int> off, idx;
    orb_featvec fv;
    explicit Csr(const FeatureVector* f) {
        off.push_back(0);
        if (f)
            for (FeatureVector::const_iterator it = f->begin(); it != f->end(); ++it) {
                ids.push_back(it->first);
                for (size_t j = 0; j < it->second.size(); j++) idx.push_back((int)it->second[j]);
                off.push_back((int)idx.size());
            }
        if (idx.empty()) idx.push_back(0);
        fv.nnodes = (int)ids.size();
        fv.node_ids = ids.empty() ? nullptr : ids.data();
        fv.offsets = off.data();
        fv.indices = idx.data();
    }
};

std::vector<float> angles(const FeatureSet& s) {
    std::vector<float> a(std::max(s.N(), 1), 0.f);
    for (int i = 0; i < s.N(); i++) a[i] = s.keys[i].angle;
    return a;
}

// mvuRight gates the search: the FeatureSet's array, or the resident frame's
bool has_uright(const FeatureSet& s) { return s.resident ? s.resident->hasURight() : s.uRight != nullptr; }

const uint8_t* desc_ptr(const FeatureSet& s) {
    static const uint8_t dummy[32] = {0};
    return (s.descriptors && s.N()) ? s.descriptors : dummy;
}

const KeyPoint* keys_ptr(const FeatureSet& s) {
    static const KeyPoint dummy = {0, 0, 0, 0, 0, 0, 0};
    return (s.keys && s.N()) ? s.keys : &dummy;
}

void require(bool ok, const char* what) {
    if (!ok) throw OrbGpuError(ORB_ERR_ARG, what);
}

std::vector<uint8_t> flags_or(const uint8_t* v, int n, uint8_t dflt) {
    return v ? std::vector<uint8_t>(v, v + n) : std::vector<uint8_t>(n, dflt);
}

std::vector<float> floats_or(const float* v, int n, float dflt) {
    return v ? std::vector<float>(v, v + n) : std::vector<float>(n, dflt);
}

}  // namespace

/* ---------------- Frame grid (Frame.cc:378-412, 494-560, 877-940) ---------------- */
FrameGrid::FrameGrid(const KeyPoint* keysUn, int n, float minX, float maxX, float minY, float maxY) {
    minX_ = minX;
    minY_ = minY;
    invW_ = static_cast<float>(ORBGPU_FRAME_GRID_COLS) / static_cast<float>(maxX - minX);   // Frame.cc:156-157
    invH_ = static_cast<float>(ORBGPU_FRAME_GRID_ROWS) / static_cast<float>(maxY - minY);
    assign(keysUn, n);
}

FrameGrid FrameGrid::Birdview(const KeyPoint* keysBird, int n, float widthInv, float heightInv) {
    FrameGrid g;
    g.invW_ = widthInv;
    g.invH_ = heightInv;
    g.assign(keysBird, n);
    return g;
}

void FrameGrid::assign(const KeyPoint* keys, int n) {
    keys_ = keys;
    cells_.assign((size_t)ORBGPU_FRAME_GRID_COLS * ORBGPU_FRAME_GRID_ROWS, std::vector<size_t>());
    for (int i = 0; i < n; i++) {
        // PosInGrid (Frame.cc:549-560): round((x - mnMinX) * inv)
        const int posX = (int)round((keys[i].x - minX_) * invW_);
        const int posY = (int)round((keys[i].y - minY_) * invH_);
        if (posX < 0 || posX >= ORBGPU_FRAME_GRID_COLS || posY < 0 || posY >= ORBGPU_FRAME_GRID_ROWS) continue;
        cells_[(size_t)posX * ORBGPU_FRAME_GRID_ROWS + posY].push_back(i);
    }
}

std::vector<size_t> FrameGrid::GetFeaturesInArea(float x, float y, float r, int minLevel, int maxLevel) const {
    std::vector<size_t> vIndices;
    if (cells_.empty()) return vIndices;
    const int nMinCellX = std::max(0, (int)floor((x - minX_ - r) * invW_));
    if (nMinCellX >= ORBGPU_FRAME_GRID_COLS) return vIndices;
    const int nMaxCellX = std::min((int)ORBGPU_FRAME_GRID_COLS - 1, (int)ceil((x - minX_ + r) * invW_));
    if (nMaxCellX < 0) return vIndices;
    const int nMinCellY = std::max(0, (int)floor((y - minY_ - r) * invH_));
    if (nMinCellY >= ORBGPU_FRAME_GRID_ROWS) return vIndices;
    const int nMaxCellY = std::min((int)ORBGPU_FRAME_GRID_ROWS - 1, (int)ceil((y - minY_ + r) * invH_));
    if (nMaxCellY < 0) return vIndices;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
            const std::vector<size_t>& vCell = cells_[(size_t)ix * ORBGPU_FRAME_GRID_ROWS + iy];
            for (size_t j = 0; j < vCell.size(); j++) {
                const KeyPoint& kp = keys_[vCell[j]];
                if (bCheckLevels) {
                    if (kp.octave < minLevel) continue;
                    if (maxLevel >= 0 && kp.octave > maxLevel) continue;
                }
                const float distx = kp.x - x, disty = kp.y - y;
                if (fabs(distx) < r && fabs(disty) < r) vIndices.push_back(vCell[j]);
            }
        }
    return vIndices;
}

orb_frame_grid FrameGrid::Csr(std::vector<int>& off, std::vector<int>& idx) const {
    const size_t ncells = (size_t)ORBGPU_FRAME_GRID_COLS * ORBGPU_FRAME_GRID_ROWS;
    off.assign(ncells + 1, 0);
    idx.clear();
    for (size_t c = 0; c < ncells && !cells_.empty(); c++) {
        for (size_t j = 0; j < cells_[c].size(); j++) idx.push_back((int)cells_[c][j]);
        off[c + 1] = (int)idx.size();
    }
    if (idx.empty()) idx.push_back(0);
    orb_frame_grid g;
    g.min_x = minX_;
    g.min_y = minY_;
    g.inv_w = invW_;
    g.inv_h = invH_;
    g.cell_off = off.data();
    g.cell_idx = idx.data();
    return g;
}

/* ---------------- ResidentFrame (orb_frame) ---------------- */
ResidentFrame::ResidentFrame(const KeyPoint* keysUn, int n, const uint8_t* descriptors, const float* uRight, float minX,
                             float maxX, float minY, float maxY) {
    const float invW = static_cast<float>(ORBGPU_FRAME_GRID_COLS) / static_cast<float>(maxX - minX);   // as FrameGrid
    const float invH = static_cast<float>(ORBGPU_FRAME_GRID_ROWS) / static_cast<float>(maxY - minY);
    check(orb_frame_create(matcher_ctx(), n, descriptors, keysUn, uRight, minX, minY, invW, invH, &h_), "ResidentFrame");
    n_ = n;
    hasURight_ = uRight != nullptr;
}

ResidentFrame ResidentFrame::Birdview(const KeyPoint* keysBird, int n, const uint8_t* descriptors, float widthInv,
                                      float heightInv) {
    ResidentFrame f;
    check(orb_frame_create(matcher_ctx(), n, descriptors, keysBird, nullptr, 0.f, 0.f, widthInv, heightInv, &f.h_),
          "ResidentFrame::Birdview");
    f.n_ = n;
    return f;
}

ResidentFrame ResidentFrame::FromDevice(orb_ctx* ctx, int n, const uint8_t* d_descriptors, const KeyPoint* d_keysUn,
                                        const float* d_uRight, float minX, float minY, float widthInv, float heightInv) {
    ResidentFrame f;
    check(orb_frame_create_device(ctx, n, d_descriptors, d_keysUn, d_uRight, minX, minY, widthInv, heightInv, &f.h_),
          "ResidentFrame::FromDevice");
    f.n_ = n;
    f.hasURight_ = d_uRight != nullptr;
    return f;
}

ResidentFrame ResidentFrame::FromExtraction(orb_ctx* ctx, const orb_distortion& dist, int n, const uint8_t* d_descriptors,
                                            const KeyPoint* d_keysRaw, const float* d_uRight, float minX, float maxX,
                                            float minY, float maxY) {
    const float invW = static_cast<float>(ORBGPU_FRAME_GRID_COLS) / static_cast<float>(maxX - minX);   // as FrameGrid
    const float invH = static_cast<float>(ORBGPU_FRAME_GRID_ROWS) / static_cast<float>(maxY - minY);
    ResidentFrame f;
    check(orb_frame_create_from_extract(ctx, &dist, n, d_descriptors, d_keysRaw, d_uRight, minX, minY, invW, invH, &f.h_),
          "ResidentFrame::FromExtraction");
    f.n_ = n;
    f.hasURight_ = d_uRight != nullptr;
    return f;
}

std::vector<ResidentFrame> ResidentFrame::FromBatch(orb_ctx* ctx, const orb_distortion& dist, int nframes,
                                                    const uint8_t* d_descriptors, const KeyPoint* d_keysRaw,
                                                    const int* d_counts, int kp_cap, float minX, float maxX, float minY,
                                                    float maxY) {
    const float invW = static_cast<float>(ORBGPU_FRAME_GRID_COLS) / static_cast<float>(maxX - minX);
    const float invH = static_cast<float>(ORBGPU_FRAME_GRID_ROWS) / static_cast<float>(maxY - minY);
    std::vector<orb_frame*> h((size_t)std::max(nframes, 0), nullptr);
    std::vector<ResidentFrame> out(h.size());   // (allocated before the handles exist: nothing can throw after)
    check(orb_frames_create_from_batch(ctx, &dist, nframes, d_descriptors, d_keysRaw, d_counts, kp_cap, minX, minY, invW,
                                       invH, h.data()),
          "ResidentFrame::FromBatch");
    for (size_t f = 0; f < h.size(); f++) {
        out[f].h_ = h[f];
        out[f].n_ = orb_frame_count(h[f]);
    }
    return out;
}

std::vector<ResidentFrame> ResidentFrame::FromBatchRGBD(orb_ctx* ctx, const orb_distortion& dist,
                                                        const orb_depth_map& depth, float mbf, int nframes,
                                                        const uint8_t* d_descriptors, const KeyPoint* d_keysRaw,
                                                        const int* d_counts, int kp_cap, float minX, float maxX,
                                                        float minY, float maxY, float* d_uRight, float* d_depth) {
    const float invW = static_cast<float>(ORBGPU_FRAME_GRID_COLS) / static_cast<float>(maxX - minX);
    const float invH = static_cast<float>(ORBGPU_FRAME_GRID_ROWS) / static_cast<float>(maxY - minY);
    std::vector<orb_frame*> h((size_t)std::max(nframes, 0), nullptr);
    std::vector<ResidentFrame> out(h.size());   // (allocated before the handles exist: nothing can throw after)
    check(orb_frames_create_from_batch_rgbd(ctx, &dist, &depth, mbf, nframes, d_descriptors, d_keysRaw, d_counts, kp_cap,
                                            minX, minY, invW, invH, d_uRight, d_depth, h.data()),
          "ResidentFrame::FromBatchRGBD");
    for (size_t f = 0; f < h.size(); f++) {
        out[f].h_ = h[f];
        out[f].n_ = orb_frame_count(h[f]);
        out[f].hasURight_ = true;
    }
    return out;
}

std::vector<ResidentFrame> ResidentFrame::FromBatchStereo(orb_ctx* ctx, const orb_distortion& dist, int npairs, float mb,
                                                          float mbf, const uint8_t* d_descriptors,
                                                          const KeyPoint* d_keysRaw, const int* d_counts, int kp_cap,
                                                          float minX, float maxX, float minY, float maxY,
                                                          float* d_uRight, float* d_depth) {
    const float invW = static_cast<float>(ORBGPU_FRAME_GRID_COLS) / static_cast<float>(maxX - minX);
    const float invH = static_cast<float>(ORBGPU_FRAME_GRID_ROWS) / static_cast<float>(maxY - minY);
    std::vector<orb_frame*> h((size_t)std::max(npairs, 0), nullptr);
    std::vector<ResidentFrame> out(h.size());   // (allocated before the handles exist: nothing can throw after)
    check(orb_frames_create_from_batch_stereo(ctx, &dist, npairs, mb, mbf, d_descriptors, d_keysRaw, d_counts, kp_cap,
                                              minX, minY, invW, invH, d_uRight, d_depth, h.data()),
          "ResidentFrame::FromBatchStereo");
    for (size_t f = 0; f < h.size(); f++) {
        out[f].h_ = h[f];
        out[f].n_ = orb_frame_count(h[f]);
        out[f].hasURight_ = true;
    }
    return out;
}

namespace {
orb_distortion distortion_of(float fx, float fy, float cx, float cy, const float distCoef[4]) {
    orb_distortion d;
    d.fx = fx;
    d.fy = fy;
    d.cx = cx;
    d.cy = cy;
    for (int k = 0; k < 4; k++) d.k[k] = distCoef[k];
    return d;
}
}  // namespace

std::vector<KeyPoint> UndistortKeyPoints(float fx, float fy, float cx, float cy, const float distCoef[4],
                                         const std::vector<KeyPoint>& keys) {
    const orb_distortion d = distortion_of(fx, fy, cx, cy, distCoef);
    std::vector<KeyPoint> keysUn(keys.size());
    check(orb_undistort_keypoints(matcher_ctx(), &d, (int)keys.size(), keys.data(), keysUn.data(), nullptr),
          "UndistortKeyPoints");
    return keysUn;
}

void ComputeImageBounds(float fx, float fy, float cx, float cy, const float distCoef[4], int cols, int rows, float& minX,
                        float& maxX, float& minY, float& maxY) {
    const orb_distortion d = distortion_of(fx, fy, cx, cy, distCoef);
    check(orb_image_bounds(&d, cols, rows, &minX, &maxX, &minY, &maxY), "ComputeImageBounds");
}

ResidentFrame::~ResidentFrame() { orb_frame_destroy(h_); }

ResidentFrame::ResidentFrame(ResidentFrame&& o) noexcept
    : h_(o.h_), n_(o.n_), hasURight_(o.hasURight_), fvCap_(o.fvCap_) {
    o.h_ = nullptr;
    o.n_ = 0;
    o.hasURight_ = false;
}

ResidentFrame& ResidentFrame::operator=(ResidentFrame&& o) noexcept {
    if (this != &o) {
        orb_frame_destroy(h_);
        h_ = o.h_;
        n_ = o.n_;
        hasURight_ = o.hasURight_;
        fvCap_ = o.fvCap_;
        o.h_ = nullptr;
        o.n_ = 0;
        o.hasURight_ = false;
    }
    return *this;
}

/* ---------------- ResidentPoints (orb_points) ---------------- */
ResidentPoints::ResidentPoints(int capacity) {
    check(orb_points_create(matcher_ctx(), capacity, &h_), "ResidentPoints");
}

ResidentPoints::~ResidentPoints() { orb_points_destroy(h_); }

ResidentPoints::ResidentPoints(ResidentPoints&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }

ResidentPoints& ResidentPoints::operator=(ResidentPoints&& o) noexcept {
    if (this != &o) {
        orb_points_destroy(h_);
        h_ = o.h_;
        o.h_ = nullptr;
    }
    return *this;
}

void ResidentPoints::Write(int first, int n, const float* pos, const float* normal, const float* minDistance,
                           const float* maxDistance, const uint8_t* descriptors) {
    check(orb_points_write(h_, first, n, pos, normal, minDistance, maxDistance, descriptors), "ResidentPoints::Write");
}

void ResidentFrame::Grid(std::vector<int>& off, std::vector<int>& idx) const {
    require(h_ != nullptr, "ResidentFrame::Grid: empty handle");
    off.assign((size_t)ORBGPU_FRAME_GRID_COLS * ORBGPU_FRAME_GRID_ROWS + 1, 0);
    idx.assign(std::max(n_, 1), 0);
    int nslots = 0;
    check(orb_frame_grid_read(h_, off.data(), idx.data(), n_, &nslots), "ResidentFrame::Grid");
    idx.resize(nslots);
}

void ResidentFrame::ComputeBoW(orb_ctx* ctx, const orb_vocab* vocab, int levelsup) {
    require(h_ != nullptr, "ResidentFrame::ComputeBoW: empty handle");
    orb_frame* one = h_;
    check(orb_frame_compute_bow(ctx, vocab, levelsup, 1, &one), "ResidentFrame::ComputeBoW");
    fvCap_ = 0;
}

void ResidentFrame::ComputeBoW(orb_ctx* ctx, const orb_vocab* vocab, const std::vector<ResidentFrame*>& frames,
                               int levelsup) {
    std::vector<orb_frame*> h(frames.size());
    for (size_t f = 0; f < frames.size(); f++) {
        require(frames[f] && frames[f]->h_, "ResidentFrame::ComputeBoW: empty handle");
        h[f] = frames[f]->h_;
    }
    check(orb_frame_compute_bow(ctx, vocab, levelsup, (int)h.size(), h.data()), "ResidentFrame::ComputeBoW(batch)");
    for (ResidentFrame* f : frames) f->fvCap_ = 0;
}

void ResidentFrame::SetFeatVec(const FeatureVector& featVec) {
    require(h_ != nullptr, "ResidentFrame::SetFeatVec: empty handle");
    Csr a(&featVec);
    check(orb_frame_set_featvec(matcher_ctx(), h_, a.fv), "ResidentFrame::SetFeatVec");
    fvCap_ = std::max(a.ids.size(), a.idx.size());
}

void ResidentFrame::BoW(const orb_vocab* vocab, std::map<unsigned int, double>& bowVec, FeatureVector& featVec) const {
    require(h_ != nullptr, "ResidentFrame::BoW: empty handle");
    // (a FeatureVector given by SetFeatVec may hold more entries than features)
    const size_t nw = (size_t)std::max(n_, 1), cap = std::max(nw, fvCap_);
    std::vector<int> words(nw), off(cap + 1), idx(cap);
    std::vector<double> values(nw);
    std::vector<uint32_t> nodes(cap);
    int nb = 0, nf = 0;
    check(orb_frame_bow_read(vocab, h_, words.data(), values.data(), &nb, nodes.data(), off.data(), idx.data(), &nf),
          "ResidentFrame::BoW");
    bowVec.clear();
    featVec.clear();
    for (int i = 0; i < nb; i++) bowVec[(unsigned int)words[i]] = values[i];
    for (int j = 0; j < nf; j++)
        featVec[nodes[j]] = std::vector<unsigned int>(idx.begin() + off[j], idx.begin() + off[j + 1]);
}

namespace {
// the train side's handle, checked against the FeatureSet it stands for (NULL: the FrameGrid form)
const orb_frame* resident_of(const FeatureSet& F, const char* what) {
    if (!F.resident) return nullptr;
    require(F.resident->handle() != nullptr && F.resident->N() == F.N(), what);
    return F.resident->handle();
}
}  // namespace

/* ---------------- ORBmatcher ---------------- */
ORBmatcher::ORBmatcher(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

int ORBmatcher::DescriptorDistance(const uint8_t* a, const uint8_t* b) { return orb_descriptor_distance(a, b); }

int ORBmatcher::SearchByBoW(const KeyFrameData& KF, const FrameData& F, std::vector<int>& vpMapPointMatches) {
    const int nKF = KF.N(), nF = F.N();
    vpMapPointMatches.assign(nF, -1);   // :163 vector<MapPoint*>(F.N, NULL)
    Csr a(KF.featVec), b(F.featVec);
    require(nKF == 0 || (KF.keys && KF.descriptors), "SearchByBoW: KF keys/descriptors");
    require(nF == 0 || (F.keys && F.descriptors), "SearchByBoW: F keys/descriptors");
    std::vector<float> angKF = angles(KF), angF = angles(F);
    std::vector<uint8_t> mp = flags_or(KF.hasMapPoint, std::max(nKF, 1), 1);
    std::vector<int> out(std::max(nF, 1), -1);
    int nmatches = 0;
    check(orb_search_by_bow_kf_f(matcher_ctx(), mfNNratio, mbCheckOrientation, nKF, desc_ptr(KF), angKF.data(),
                                 mp.data(), a.fv, nF, desc_ptr(F), angF.data(), b.fv, out.data(), &nmatches),
          "SearchByBoW(KF,F)");
    std::copy(out.begin(), out.begin() + nF, vpMapPointMatches.begin());
    return nmatches;
}

int ORBmatcher::SearchByBoW(const KeyFrameData& KF1, const KeyFrameData& KF2, std::vector<int>& vpMatches12) {
    const int n1 = KF1.N(), n2 = KF2.N();
    vpMatches12.assign(n1, -1);   // :535
    Csr a(KF1.featVec), b(KF2.featVec);
    require(n1 == 0 || (KF1.keys && KF1.descriptors), "SearchByBoW: KF1 keys/descriptors");
    require(n2 == 0 || (KF2.keys && KF2.descriptors), "SearchByBoW: KF2 keys/descriptors");
    std::vector<float> ang1 = angles(KF1), ang2 = angles(KF2);
    std::vector<uint8_t> mp1 = flags_or(KF1.hasMapPoint, std::max(n1, 1), 1),
                         mp2 = flags_or(KF2.hasMapPoint, std::max(n2, 1), 1);
    std::vector<int> out(std::max(n1, 1), -1);
    int nmatches = 0;
    check(orb_search_by_bow_kf_kf(matcher_ctx(), mfNNratio, mbCheckOrientation, n1, desc_ptr(KF1), ang1.data(),
                                  mp1.data(), a.fv, n2, desc_ptr(KF2), ang2.data(), mp2.data(), b.fv, out.data(),
                                  &nmatches),
          "SearchByBoW(KF,KF)");
    std::copy(out.begin(), out.begin() + n1, vpMatches12.begin());
    return nmatches;
}

int ORBmatcher::SearchForTriangulation(const KeyFrameData& KF1, const KeyFrameData& KF2, const float F12[9], float ex,
                                       float ey, std::vector<std::pair<size_t, size_t> >& vMatchedPairs,
                                       const bool bOnlyStereo) {
    const int n1 = KF1.N(), n2 = KF2.N();
    Csr a(KF1.featVec), b(KF2.featVec);
    require(n1 == 0 || (KF1.keys && KF1.descriptors), "SearchForTriangulation: KF1 keys/descriptors");
    require(n2 == 0 || (KF2.keys && KF2.descriptors), "SearchForTriangulation: KF2 keys/descriptors");
    require(KF2.scaleFactors && KF2.levelSigma2 && KF2.nlevels > 0, "SearchForTriangulation: KF2 scale tables");
    std::vector<uint8_t> mp1 = flags_or(KF1.hasMapPoint, std::max(n1, 1), 0),
                         mp2 = flags_or(KF2.hasMapPoint, std::max(n2, 1), 0);
    std::vector<float> ur1 = floats_or(KF1.uRight, std::max(n1, 1), -1.f), ur2 = floats_or(KF2.uRight, std::max(n2, 1), -1.f);
    std::vector<int> pairs(2 * (size_t)std::max(n1, 1));
    int np = 0;
    check(orb_search_for_triangulation(matcher_ctx(), mbCheckOrientation, bOnlyStereo, n1, desc_ptr(KF1), keys_ptr(KF1),
                                       mp1.data(), ur1.data(), a.fv, n2, desc_ptr(KF2), keys_ptr(KF2), mp2.data(),
                                       ur2.data(), b.fv, F12, ex, ey, KF2.scaleFactors, KF2.levelSigma2,
                                       KF2.nlevels, pairs.data(),
                                       std::max(n1, 1), &np),
          "SearchForTriangulation");
    vMatchedPairs.clear();   // :813-820
    vMatchedPairs.reserve(np);
    for (int i = 0; i < np; i++) vMatchedPairs.push_back(std::make_pair((size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]));
    return np;
}

int ORBmatcher::SearchForTriangulation(const KeyFrameData& KF1, const std::vector<TriangulationNeighbour>& neighbours,
                                       std::vector<std::vector<std::pair<size_t, size_t> > >& vvMatchedPairs,
                                       const bool bOnlyStereo) {
    const int n1 = KF1.N(), np = (int)neighbours.size();
    require(n1 == 0 || (KF1.keys && KF1.descriptors), "SearchForTriangulation: KF1 keys/descriptors");
    Csr a(KF1.featVec);
    std::vector<uint8_t> mp1 = flags_or(KF1.hasMapPoint, std::max(n1, 1), 0);
    std::vector<float> ur1 = floats_or(KF1.uRight, std::max(n1, 1), -1.f);
    struct Side {   // one neighbour's views, alive until the call returns
        std::vector<uint8_t> mp;
        std::vector<float> ur;
        std::vector<int> pairs;
        int n = 0;
    };
    std::vector<Side> side(np);
    std::vector<Csr> csr;
    csr.reserve(np);
    std::vector<orb_tri_pair> P(np);
    for (int p = 0; p < np; p++) {
        require(neighbours[p].KF2 != nullptr, "SearchForTriangulation: neighbour KeyFrame");
        const KeyFrameData& KF2 = *neighbours[p].KF2;
        const int n2 = KF2.N();
        require(n2 == 0 || (KF2.keys && KF2.descriptors), "SearchForTriangulation: KF2 keys/descriptors");
        require(KF2.scaleFactors && KF2.levelSigma2 && KF2.nlevels > 0, "SearchForTriangulation: KF2 scale tables");
        Side& sd = side[p];
        sd.mp = flags_or(KF2.hasMapPoint, std::max(n2, 1), 0);
        sd.ur = floats_or(KF2.uRight, std::max(n2, 1), -1.f);
        sd.pairs.resize(2 * (size_t)std::max(n1, 1));
        csr.emplace_back(KF2.featVec);
        P[p] = orb_tri_pair{n2, desc_ptr(KF2), keys_ptr(KF2), sd.mp.data(), sd.ur.data(), csr.back().fv,
                            neighbours[p].F12, neighbours[p].ex, neighbours[p].ey, KF2.scaleFactors, KF2.levelSigma2,
                            KF2.nlevels, sd.pairs.data(), std::max(n1, 1), &sd.n};
    }
    check(orb_search_for_triangulation_batch(matcher_ctx(), mbCheckOrientation, bOnlyStereo, n1, desc_ptr(KF1),
                                             keys_ptr(KF1), mp1.data(), ur1.data(), a.fv, np, P.data()),
          "SearchForTriangulation(batch)");
    vvMatchedPairs.assign(np, std::vector<std::pair<size_t, size_t> >());
    int total = 0;
    for (int p = 0; p < np; p++) {
        for (int i = 0; i < side[p].n; i++)
            vvMatchedPairs[p].push_back(std::make_pair((size_t)side[p].pairs[2 * i], (size_t)side[p].pairs[2 * i + 1]));
        total += side[p].n;
    }
    return total;
}

int ORBmatcher::window_match(bool level0_only, const FeatureSet& F1, const FeatureSet& F2,
                             const std::vector<Point2f>* centres, int windowSize, std::vector<int>& vnMatches12) {
    const int n1 = F1.N(), n2 = F2.N();
    vnMatches12.assign(n1, -1);
    require(n1 == 0 || (F1.keys && F1.descriptors), "window match: F1 keys/descriptors");
    if (const orb_frame* R = resident_of(F2, "window match: F2 resident frame")) {
        // GetFeaturesInArea on the device over the handle's grid: the same candidates in the same order
        std::vector<float> cen;
        if (centres) {
            require((int)centres->size() >= n1, "window match: one centre per F1 feature");
            cen.resize(2 * (size_t)std::max(n1, 1));
            for (int i = 0; i < n1; i++) {
                cen[2 * i] = (*centres)[i].x;
                cen[2 * i + 1] = (*centres)[i].y;
            }
        }
        std::vector<int> out(std::max(n1, 1), -1);
        int nmatches = 0;
        check(orb_window_match_frame(matcher_ctx(), mfNNratio, mbCheckOrientation, level0_only, n1, desc_ptr(F1),
                                     keys_ptr(F1), centres ? cen.data() : nullptr, (float)windowSize, R, out.data(),
                                     &nmatches),
              "window match (resident)");
        std::copy(out.begin(), out.begin() + n1, vnMatches12.begin());
        return nmatches;
    }
    require(F2.grid != nullptr, "window match: F2 grid");
    require(n2 == 0 || (F2.keys && F2.descriptors), "window match: F2 keys/descriptors");
    // candidate lists: F2.GetFeaturesInArea(centre, windowSize, level1, level1) per query (:425, :1686, :1806)
    std::vector<int> off(n1 + 1, 0), idx;
    for (int i1 = 0; i1 < n1; i1++) {
        const KeyPoint& kp1 = F1.keys[i1];
        if (!(level0_only && kp1.octave > 0)) {
            const float x = centres ? (*centres)[i1].x : kp1.x, y = centres ? (*centres)[i1].y : kp1.y;
            const std::vector<size_t> v = F2.grid->GetFeaturesInArea(x, y, (float)windowSize, kp1.octave, kp1.octave);
            for (size_t j = 0; j < v.size(); j++) idx.push_back((int)v[j]);
        }
        off[i1 + 1] = (int)idx.size();
    }
    if (idx.empty()) idx.push_back(0);
    std::vector<int> out(std::max(n1, 1), -1);
    int nmatches = 0;
    check(orb_window_match(matcher_ctx(), mfNNratio, mbCheckOrientation, level0_only, n1, desc_ptr(F1), keys_ptr(F1),
                           n2, desc_ptr(F2), keys_ptr(F2), off.data(), idx.data(), out.data(), &nmatches),
          "window match");
    std::copy(out.begin(), out.begin() + n1, vnMatches12.begin());
    return nmatches;
}

int ORBmatcher::SearchForInitialization(const FrameData& F1, const FrameData& F2, std::vector<Point2f>& vbPrevMatched,
                                        std::vector<int>& vnMatches12, int windowSize) {
    const int n = window_match(true, F1, F2, &vbPrevMatched, windowSize, vnMatches12);
    for (size_t i1 = 0; i1 < vnMatches12.size(); i1++)   // :514-517 update prev matched
        if (vnMatches12[i1] >= 0) {
            const KeyPoint& k = F2.keys[vnMatches12[i1]];
            vbPrevMatched[i1].x = k.x;
            vbPrevMatched[i1].y = k.y;
        }
    return n;
}

int ORBmatcher::BirdviewMatch(const FrameData& F1, const FrameData& F2, std::vector<int>& vnMatches12,
                              std::vector<Point2f>& vPrevMatched, int windowSize) {
    const int n = window_match(true, F1, F2, &vPrevMatched, windowSize, vnMatches12);
    for (size_t i1 = 0; i1 < vnMatches12.size(); i1++)   // :1778-1781
        if (vnMatches12[i1] >= 0) {
            const KeyPoint& k = F2.keys[vnMatches12[i1]];
            vPrevMatched[i1].x = k.x;
            vPrevMatched[i1].y = k.y;
        }
    return n;
}

int ORBmatcher::BirdviewMatch(const FrameData& F1, const FrameData& F2, std::vector<int>& vnMatches12,
                              int windowSize) {
    return window_match(false, F1, F2, nullptr, windowSize, vnMatches12);
}

/* ---------------- projection-gated searches (orb_search_by_projection) ---------------- */
int ORBmatcher::projection_search(int mode, const FeatureSet& F, bool stereo, const std::vector<orb_proj_query>& q,
                                  const std::vector<uint8_t>& qdesc, std::vector<int>& matches, const char* what,
                                  int max_dist, int check_ori, const uint8_t* taken) {
    const int n = F.N(), nq = (int)q.size();
    matches.assign(n, -1);
    if (const orb_frame* R = resident_of(F, "projection search: resident frame")) {
        require(!stereo || F.resident->hasURight(), "projection search: resident frame without uRight");
        std::vector<int> out(std::max(n, 1), -1);
        int nmatches = 0;
        check(orb_search_by_projection_frame(matcher_ctx(), mode, mfNNratio,
                                             check_ori < 0 ? (int)mbCheckOrientation : check_ori,
                                             max_dist < 0 ? TH_HIGH : max_dist, nq, nq ? q.data() : nullptr,
                                             nq ? qdesc.data() : nullptr, R, taken ? taken : F.hasMapPoint, stereo ? 1 : 0,
                                             out.data(), &nmatches),
              what);
        std::copy(out.begin(), out.begin() + n, matches.begin());
        return nmatches;
    }
    require(F.grid != nullptr, "projection search: Frame grid");
    require(n == 0 || (F.keys && F.descriptors), "projection search: Frame keys/descriptors");
    std::vector<int> off, idx;
    const orb_frame_grid g = F.grid->Csr(off, idx);
    std::vector<int> out(std::max(n, 1), -1);
    int nmatches = 0;
    check(orb_search_by_projection(matcher_ctx(), mode, mfNNratio, check_ori < 0 ? (int)mbCheckOrientation : check_ori,
                                   max_dist < 0 ? TH_HIGH : max_dist, nq, nq ? q.data() : nullptr,
                                   nq ? qdesc.data() : nullptr, n, desc_ptr(F), keys_ptr(F), stereo ? F.uRight : nullptr,
                                   taken ? taken : F.hasMapPoint, g, out.data(), &nmatches),
          what);
    std::copy(out.begin(), out.begin() + n, matches.begin());
    return nmatches;
}

int ORBmatcher::SearchByProjection(FrameData& CurrentFrame, const ProjectedLastFrame& LastFrame, const float th,
                                   const bool bMono, std::vector<int>& vpMapPointMatches) {
    const size_t nq = LastFrame.points.size();
    require(nq == 0 || (CurrentFrame.scaleFactors && CurrentFrame.nlevels > 0), "SearchByProjection: scale table");
    const bool bForward = LastFrame.bForward && !bMono, bBackward = LastFrame.bBackward && !bMono;   // :1348-1349
    std::vector<orb_proj_query> q(nq);
    std::vector<uint8_t> qdesc(nq * 32);
    for (size_t i = 0; i < nq; i++) {
        const ProjectedLastFrame::Point& p = LastFrame.points[i];
        require(p.descriptor && p.octave >= 0 && p.octave < CurrentFrame.nlevels, "SearchByProjection: map point");
        const float radius = th * CurrentFrame.scaleFactors[p.octave];   // :1381
        q[i].u = p.u;
        q[i].v = p.v;
        q[i].r = radius;
        if (bForward) {                                                  // :1385-1390
            q[i].min_level = p.octave;
            q[i].max_level = -1;
        } else if (bBackward) {
            q[i].min_level = 0;
            q[i].max_level = p.octave;
        } else {
            q[i].min_level = p.octave - 1;
            q[i].max_level = p.octave + 1;
        }
        const float disp = LastFrame.mbf * p.invzc;
        q[i].ur = p.u - disp;                                            // :1409
        q[i].ur_tol = radius;                                            // :1411
        q[i].angle = p.angle;
        q[i].blocks = p.observed ? 1 : 0;
        memcpy(&qdesc[i * 32], p.descriptor, 32);
    }
    return projection_search(ORB_PROJ_BEST, CurrentFrame, has_uright(CurrentFrame), q, qdesc, vpMapPointMatches,
                             "SearchByProjection(CurrentFrame, LastFrame)");
}

int ORBmatcher::SearchByProjection(FrameData& F, const ProjectedMapPoints& vpMapPoints, const float th,
                                   std::vector<int>& vpMapPointMatches) {
    const size_t nq = vpMapPoints.points.size();
    require(nq == 0 || (F.scaleFactors && F.nlevels > 0), "SearchByProjection: scale table");
    const bool bFactor = th != 1.0;                                      // :49
    std::vector<orb_proj_query> q(nq);
    std::vector<uint8_t> qdesc(nq * 32);
    for (size_t i = 0; i < nq; i++) {
        const ProjectedMapPoints::Point& p = vpMapPoints.points[i];
        require(p.descriptor && p.level >= 0 && p.level < F.nlevels, "SearchByProjection: map point");
        float r = p.viewCos > 0.998 ? 2.5f : 4.0f;                       // RadiusByViewingCos, :131-137
        if (bFactor) r *= th;                                            // :65-66
        const float rr = r * F.scaleFactors[p.level];                    // :69, :94
        q[i].u = p.projX;
        q[i].v = p.projY;
        q[i].r = rr;
        q[i].min_level = p.level - 1;
        q[i].max_level = p.level;
        q[i].ur = p.projXR;
        q[i].ur_tol = rr;
        q[i].angle = 0;
        q[i].blocks = 1;
        memcpy(&qdesc[i * 32], p.descriptor, 32);
    }
    return projection_search(ORB_PROJ_RATIO_SAME_LEVEL, F, has_uright(F), q, qdesc, vpMapPointMatches,
                             "SearchByProjection(F, MapPoints)");
}

int ORBmatcher::SearchByProjectionBird(FrameData& F, const ProjectedBirdPoints& vpMapPointsBird, const float r,
                                       std::vector<int>& vpMapPointMatchesBird) {
    const size_t nq = vpMapPointsBird.points.size();
    std::vector<orb_proj_query> q(nq);
    std::vector<uint8_t> qdesc(nq * 32);
    for (size_t i = 0; i < nq; i++) {
        const ProjectedBirdPoints::Point& p = vpMapPointsBird.points[i];
        require(p.descriptor != nullptr, "SearchByProjectionBird: map point");
        q[i].u = p.x;
        q[i].v = p.y;
        q[i].r = r;
        q[i].min_level = -1;   // GetFeaturesInAreaBirdview(pt.x, pt.y, r): the default levels (:1945)
        q[i].max_level = -1;
        q[i].ur = 0;
        q[i].ur_tol = 0;
        q[i].angle = 0;
        q[i].blocks = 1;
        memcpy(&qdesc[i * 32], p.descriptor, 32);
    }
    return projection_search(ORB_PROJ_RATIO_SAME_LEVEL, F, false, q, qdesc, vpMapPointMatchesBird,
                             "SearchByProjectionBird");
}

/* ---------------- SearchByMatchBird (orb_search_by_match_bird, orb_search_by_match_bird_frame) ---------------- */
int ORBmatcher::SearchByMatchBird(const KeyFrameBirdPoints& KF, FrameData& F, std::vector<int>& vpMapPointMatchesBird,
                                  const float r) {
    const int n = F.N(), nq = (int)KF.points.size();
    vpMapPointMatchesBird.assign(n, -1);   // :2004 vector<MapPointBird*>(F.mvKeysBird.size(), NULL)
    const orb_frame* R = resident_of(F, "SearchByMatchBird: resident frame");
    require(R || F.grid != nullptr, "SearchByMatchBird: Frame grid");
    require(R || n == 0 || (F.keys && F.descriptors), "SearchByMatchBird: Frame keys/descriptors");
    std::vector<int> id(nq);
    std::vector<float> xy(2 * (size_t)nq), angle(nq);
    std::vector<uint8_t> qdesc((size_t)nq * 32);
    for (int i = 0; i < nq; i++) {
        const KeyFrameBirdPoints::Point& p = KF.points[i];
        require(p.descriptor != nullptr && p.index >= 0, "SearchByMatchBird: keyframe point");
        id[i] = p.index;
        xy[2 * i] = p.x;
        xy[2 * i + 1] = p.y;
        angle[i] = p.angle;
        memcpy(&qdesc[(size_t)i * 32], p.descriptor, 32);
    }
    std::vector<int> out(std::max(n, 1), -1);
    int nmatches = 0;
    if (R) {
        check(orb_search_by_match_bird_resident(matcher_ctx(), mfNNratio, mbCheckOrientation, TH_HIGH, r, nq,
                                                nq ? id.data() : nullptr, nq ? xy.data() : nullptr,
                                                nq ? angle.data() : nullptr, nq ? qdesc.data() : nullptr, R, out.data(),
                                                &nmatches),
              "SearchByMatchBird(KF, F) (resident)");
        std::copy(out.begin(), out.begin() + n, vpMapPointMatchesBird.begin());
        return nmatches;
    }
    std::vector<int> off, idx;
    const orb_frame_grid g = F.grid->Csr(off, idx);
    check(orb_search_by_match_bird(matcher_ctx(), mfNNratio, mbCheckOrientation, TH_HIGH, r, nq, nq ? id.data() : nullptr,
                                   nq ? xy.data() : nullptr, nq ? angle.data() : nullptr, nq ? qdesc.data() : nullptr, n,
                                   desc_ptr(F), keys_ptr(F), g, out.data(), &nmatches),
          "SearchByMatchBird(KF, F)");
    std::copy(out.begin(), out.begin() + n, vpMapPointMatchesBird.begin());
    return nmatches;
}

int ORBmatcher::SearchByMatchBird(FrameData& CurrentFrame, const FrameData& LastFrame, const int windowSize,
                                  std::vector<int>& vpMapPointsBird) {
    const int nc = CurrentFrame.N(), nl = LastFrame.N();
    vpMapPointsBird.assign(nc, -1);
    require(CurrentFrame.grid != nullptr, "SearchByMatchBird: CurrentFrame grid");
    require(nc == 0 || (CurrentFrame.keys && CurrentFrame.descriptors), "SearchByMatchBird: CurrentFrame keys/descriptors");
    require(nl == 0 || (LastFrame.keys && LastFrame.descriptors), "SearchByMatchBird: LastFrame keys/descriptors");
    std::vector<int> off, idx;
    const orb_frame_grid g = CurrentFrame.grid->Csr(off, idx);
    std::vector<int> out(std::max(nc, 1), -1);
    int nmatches = 0;
    check(orb_search_by_match_bird_frame(matcher_ctx(), mfNNratio, mbCheckOrientation, (float)windowSize, nl,
                                         desc_ptr(LastFrame), keys_ptr(LastFrame), LastFrame.hasMapPoint, nc,
                                         desc_ptr(CurrentFrame), keys_ptr(CurrentFrame), g, out.data(), &nmatches),
          "SearchByMatchBird(CurrentFrame, LastFrame)");
    std::copy(out.begin(), out.begin() + nc, vpMapPointsBird.begin());
    return nmatches;
}

/* ---------------- the keyframe searches (orb_project_best_batch, orb_search_by_projection) ---------------- */
namespace {
// A target's marshalled arrays; the orb_proj_target points into them.
struct TargetArrays {
    std::vector<orb_proj_query> q;
    std::vector<uint8_t> qdesc;
    std::vector<int> off, idx, best_idx, best_dist;
};
orb_proj_query kf_query(const ProjectedKFPoint& p, float radius, int level_above, float angle) {
    orb_proj_query q;
    q.u = p.u;
    q.v = p.v;
    q.r = radius;
    q.min_level = p.predictedLevel - 1;              // kpLevel<nPredictedLevel-1 || kpLevel>nPredictedLevel
    q.max_level = p.predictedLevel + level_above;
    q.ur = p.ur;
    q.ur_tol = 0;
    q.angle = angle;
    q.blocks = 1;
    return q;
}
// the queries and outputs of a target (both forms of the train side)
void fill_queries(const KeyFrameData& kf, const std::vector<ProjectedKFPoint>& points, bool chi2Gate, TargetArrays& a);
orb_proj_target make_target(const KeyFrameData& kf, const std::vector<ProjectedKFPoint>& points, bool chi2Gate,
                            TargetArrays& a) {
    require(kf.grid != nullptr, "keyframe search: KeyFrame grid");
    require(kf.n == 0 || (kf.keys && kf.descriptors), "keyframe search: KeyFrame keys/descriptors");
    fill_queries(kf, points, chi2Gate, a);
    orb_proj_target t;
    t.nq = (int)points.size();
    t.q = a.q.data();
    t.qdesc = a.qdesc.data();
    t.nt = kf.n;
    t.tdesc = desc_ptr(kf);
    t.kps_t = keys_ptr(kf);
    t.t_uright = chi2Gate ? kf.uRight : nullptr;
    t.inv_sigma2 = chi2Gate ? kf.invLevelSigma2 : nullptr;
    t.nlevels = chi2Gate ? kf.nlevels : 0;
    t.grid = kf.grid->Csr(a.off, a.idx);
    t.best_idx = a.best_idx.data();
    t.best_dist = a.best_dist.data();
    return t;
}
// the same target with the keyframe as a ResidentFrame (kf.resident)
orb_proj_frame_target make_frame_target(const KeyFrameData& kf, const std::vector<ProjectedKFPoint>& points,
                                        bool chi2Gate, TargetArrays& a) {
    fill_queries(kf, points, chi2Gate, a);
    orb_proj_frame_target t;
    t.nq = (int)points.size();
    t.q = a.q.data();
    t.qdesc = a.qdesc.data();
    t.frame = resident_of(kf, "keyframe search: resident frame");
    t.inv_sigma2 = chi2Gate ? kf.invLevelSigma2 : nullptr;
    t.nlevels = chi2Gate ? kf.nlevels : 0;
    t.best_idx = a.best_idx.data();
    t.best_dist = a.best_dist.data();
    return t;
}
void fill_queries(const KeyFrameData& kf, const std::vector<ProjectedKFPoint>& points, bool chi2Gate, TargetArrays& a) {
    const size_t nq = points.size();
    require(!chi2Gate || (kf.invLevelSigma2 && kf.nlevels > 0), "Fuse: mvInvLevelSigma2");
    a.q.resize(nq);
    a.qdesc.resize(nq * 32);
    for (size_t i = 0; i < nq; i++) {
        require(points[i].descriptor != nullptr, "keyframe search: map point descriptor");
        a.q[i] = kf_query(points[i], points[i].radius, 0, 0);
        memcpy(&a.qdesc[i * 32], points[i].descriptor, 32);
    }
    a.best_idx.assign(std::max<size_t>(nq, 1), -1);
    a.best_dist.assign(std::max<size_t>(nq, 1), -1);
}
// One call over targets that are all resident or all given as arrays (the C-ABI has one entry point per form).
void project_best(const std::vector<const KeyFrameData*>& kf, const std::vector<const std::vector<ProjectedKFPoint>*>& pts,
                  bool chi2Gate, std::vector<TargetArrays>& arrays, const char* what) {
    const size_t nt = kf.size();
    arrays.assign(nt, TargetArrays());
    size_t nres = 0;
    for (size_t t = 0; t < nt; t++) nres += kf[t]->resident != nullptr;
    require(nres == 0 || nres == nt, "keyframe search: every target resident, or none");
    const int gate = chi2Gate ? ORB_PROJ_GATE_FUSE : ORB_PROJ_GATE_NONE;
    if (nres) {
        std::vector<orb_proj_frame_target> T(nt);
        for (size_t t = 0; t < nt; t++) T[t] = make_frame_target(*kf[t], *pts[t], chi2Gate, arrays[t]);
        check(orb_project_best_frames(matcher_ctx(), gate, (int)nt, T.data()), what);
    } else {
        std::vector<orb_proj_target> T(nt);
        for (size_t t = 0; t < nt; t++) T[t] = make_target(*kf[t], *pts[t], chi2Gate, arrays[t]);
        check(orb_project_best_batch(matcher_ctx(), gate, (int)nt, nt ? T.data() : nullptr), what);
    }
}
}  // namespace

void ORBmatcher::FuseSearch(const std::vector<FuseTarget>& targets, bool chi2Gate,
                            std::vector<std::vector<FuseBest> >& best) {
    const size_t nt = targets.size();
    std::vector<TargetArrays> arrays;
    std::vector<const KeyFrameData*> kf(nt);
    std::vector<const std::vector<ProjectedKFPoint>*> pts(nt);
    for (size_t t = 0; t < nt; t++) {
        kf[t] = &targets[t].kf;
        pts[t] = &targets[t].points;
    }
    project_best(kf, pts, chi2Gate, arrays, "FuseSearch");
    best.assign(nt, std::vector<FuseBest>());
    for (size_t t = 0; t < nt; t++) {
        best[t].resize(targets[t].points.size());
        for (size_t i = 0; i < best[t].size(); i++) best[t][i] = FuseBest{arrays[t].best_idx[i], arrays[t].best_dist[i]};
    }
}

FuseBest ORBmatcher::FuseSearchOne(const FuseTarget& target, int point, const uint8_t* descriptor, bool chi2Gate) {
    require(point >= 0 && point < (int)target.points.size() && descriptor, "FuseSearchOne: point");
    ProjectedKFPoint p = target.points[point];
    p.descriptor = descriptor;
    TargetArrays a;
    const orb_proj_target t = make_target(target.kf, std::vector<ProjectedKFPoint>(1, p), chi2Gate, a);
    FuseBest b{-1, -1};
    check(orb_project_best_host(chi2Gate ? ORB_PROJ_GATE_FUSE : ORB_PROJ_GATE_NONE, &t, 0, &b.idx, &b.dist),
          "FuseSearchOne");
    return b;
}

int ORBmatcher::SearchBySim3(const KeyFrameData& KF1, const KeyFrameData& KF2, const ProjectedSim3Points& points1in2,
                             const ProjectedSim3Points& points2in1, std::vector<int>& vnMatch12) {
    require(points1in2.index.size() == points1in2.points.size() && points2in1.index.size() == points2in1.points.size(),
            "SearchBySim3: one index per point");
    std::vector<TargetArrays> a;
    project_best({&KF2, &KF1}, {&points1in2.points, &points2in1.points}, false, a, "SearchBySim3");
    const int N1 = KF1.N(), N2 = KF2.N();
    std::vector<int> vnMatch1(N1, -1), vnMatch2(N2, -1);                     // :1144-1145
    for (size_t k = 0; k < points1in2.points.size(); k++) {
        const int i1 = points1in2.index[k];
        require(i1 >= 0 && i1 < N1, "SearchBySim3: point index");
        if (a[0].best_idx[k] >= 0 && a[0].best_dist[k] <= TH_HIGH) vnMatch1[i1] = a[0].best_idx[k];   // :1221-1224
    }
    for (size_t k = 0; k < points2in1.points.size(); k++) {
        const int i2 = points2in1.index[k];
        require(i2 >= 0 && i2 < N2, "SearchBySim3: point index");
        if (a[1].best_idx[k] >= 0 && a[1].best_dist[k] <= TH_HIGH) vnMatch2[i2] = a[1].best_idx[k];   // :1301-1304
    }
    vnMatch12.assign(N1, -1);
    int nFound = 0;
    for (int i1 = 0; i1 < N1; i1++) {                                        // :1310-1323
        const int idx2 = vnMatch1[i1];
        if (idx2 >= 0) {
            const int idx1 = vnMatch2[idx2];
            if (idx1 == i1) {
                vnMatch12[i1] = idx2;
                nFound++;
            }
        }
    }
    return nFound;
}

int ORBmatcher::SearchByProjection(KeyFrameData& KF, const ProjectedLoopPoints& vpPoints, const int th,
                                   std::vector<int>& vpMatched) {
    const size_t nq = vpPoints.points.size();
    require((int)vpMatched.size() == KF.N(), "SearchByProjection(KF, Scw): vpMatched has one entry per feature");
    require(nq == 0 || (KF.scaleFactors && KF.nlevels > 0), "SearchByProjection(KF, Scw): scale table");
    std::vector<orb_proj_query> q(nq);
    std::vector<uint8_t> qdesc(nq * 32), taken(std::max<size_t>(vpMatched.size(), 1), 0);
    for (size_t i = 0; i < vpMatched.size(); i++) taken[i] = vpMatched[i] != -1;   // :375
    for (size_t i = 0; i < nq; i++) {
        const ProjectedKFPoint& p = vpPoints.points[i];
        require(p.descriptor && p.predictedLevel >= 0 && p.predictedLevel < KF.nlevels, "SearchByProjection(KF, Scw): map point");
        q[i] = kf_query(p, th * KF.scaleFactors[p.predictedLevel], 0, 0);   // :360, :380
        memcpy(&qdesc[i * 32], p.descriptor, 32);
    }
    std::vector<int> res;
    const int nmatches = projection_search(ORB_PROJ_BEST, KF, false, q, qdesc, res, "SearchByProjection(KF, Scw)", TH_LOW,
                                           0, taken.data());
    for (size_t i = 0; i < res.size(); i++)
        if (res[i] >= 0) vpMatched[i] = res[i];                              // :396
    return nmatches;
}

int ORBmatcher::SearchByProjection(FrameData& CurrentFrame, const ProjectedKeyFramePoints& vpPoints, const float th,
                                   const int ORBdist, std::vector<int>& vpMapPointMatches) {
    const size_t nq = vpPoints.points.size();
    require(vpPoints.angle.size() == nq, "SearchByProjection(F, KF): one angle per point");
    require(nq == 0 || (CurrentFrame.scaleFactors && CurrentFrame.nlevels > 0), "SearchByProjection(F, KF): scale table");
    std::vector<orb_proj_query> q(nq);
    std::vector<uint8_t> qdesc(nq * 32);
    for (size_t i = 0; i < nq; i++) {
        const ProjectedKFPoint& p = vpPoints.points[i];
        require(p.descriptor && p.predictedLevel >= 0 && p.predictedLevel < CurrentFrame.nlevels,
                "SearchByProjection(F, KF): map point");
        q[i] = kf_query(p, th * CurrentFrame.scaleFactors[p.predictedLevel], 1, vpPoints.angle[i]);   // :1526-1528, :1562
        memcpy(&qdesc[i * 32], p.descriptor, 32);
    }
    // the rotation cull of :1577-1596 is statement for statement that of :1448-1467, which BEST mode replays
    return projection_search(ORB_PROJ_BEST, CurrentFrame, false, q, qdesc, vpMapPointMatches, "SearchByProjection(F, KF)",
                             ORBdist);
}

/* ---------------- the vocabulary-gated searches between ResidentFrames that carry BoW ---------------- */
int ORBmatcher::SearchByBoW(const ResidentFrame& KF, const uint8_t* hasMapPointKF, const ResidentFrame& F,
                            std::vector<int>& vpMapPointMatches) {
    require(KF && F, "SearchByBoW: empty ResidentFrame");
    const int nF = F.N();
    vpMapPointMatches.assign(nF, -1);
    std::vector<int> out(std::max(nF, 1), -1);
    int nmatches = 0;
    const orb_bow_frame_kf K{KF.handle(), hasMapPointKF, out.data(), &nmatches};
    check(orb_search_by_bow_frames_kf_f(matcher_ctx(), mfNNratio, mbCheckOrientation, F.handle(), 1, &K),
          "SearchByBoW(KF,F) resident");
    std::copy(out.begin(), out.begin() + nF, vpMapPointMatches.begin());
    return nmatches;
}

int ORBmatcher::SearchByBoW(const ResidentFrame& KF1, const uint8_t* hasMapPoint1, const ResidentFrame& KF2,
                            const uint8_t* hasMapPoint2, std::vector<int>& vpMatches12) {
    require(KF1 && KF2, "SearchByBoW: empty ResidentFrame");
    const int n1 = KF1.N();
    vpMatches12.assign(n1, -1);
    std::vector<int> out(std::max(n1, 1), -1);
    int nmatches = 0;
    check(orb_search_by_bow_frames_kf_kf(matcher_ctx(), mfNNratio, mbCheckOrientation, KF1.handle(), hasMapPoint1,
                                         KF2.handle(), hasMapPoint2, out.data(), &nmatches),
          "SearchByBoW(KF,KF) resident");
    std::copy(out.begin(), out.begin() + n1, vpMatches12.begin());
    return nmatches;
}

int ORBmatcher::SearchForTriangulation(const ResidentFrame& KF1, const uint8_t* hasMapPoint1,
                                       const std::vector<ResidentTriangulationNeighbour>& neighbours,
                                       std::vector<std::vector<std::pair<size_t, size_t> > >& vvMatchedPairs,
                                       const bool bOnlyStereo) {
    require((bool)KF1, "SearchForTriangulation: empty ResidentFrame");
    const int n1 = KF1.N(), np = (int)neighbours.size();
    std::vector<std::vector<int> > pairs(np);
    std::vector<int> count(np, 0);
    std::vector<orb_tri_frame_pair> P(np);
    for (int p = 0; p < np; p++) {
        const ResidentTriangulationNeighbour& nb = neighbours[p];
        require(nb.KF2 && *nb.KF2, "SearchForTriangulation: neighbour ResidentFrame");
        pairs[p].resize(2 * (size_t)std::max(n1, 1));
        P[p] = orb_tri_frame_pair{nb.KF2->handle(), nb.hasMapPoint, nb.F12, nb.ex, nb.ey, nb.scaleFactors,
                                  nb.levelSigma2, nb.nlevels, pairs[p].data(), std::max(n1, 1), &count[p]};
    }
    check(orb_search_for_triangulation_frames(matcher_ctx(), mbCheckOrientation, bOnlyStereo, KF1.handle(), hasMapPoint1,
                                              np, P.data()),
          "SearchForTriangulation resident");
    vvMatchedPairs.assign(np, std::vector<std::pair<size_t, size_t> >());
    int total = 0;
    for (int p = 0; p < np; p++) {
        for (int i = 0; i < count[p]; i++)
            vvMatchedPairs[p].push_back(std::make_pair((size_t)pairs[p][2 * i], (size_t)pairs[p][2 * i + 1]));
        total += count[p];
    }
    return total;
}

/* ---------------- the ResidentFrame overloads: the FeatureSet forms with `resident` set ---------------- */
namespace {
FrameData with_resident(const FrameData& members, const ResidentFrame& R) {
    FrameData F = members;
    F.n = R.N();
    F.resident = &R;
    return F;
}
}  // namespace

int ORBmatcher::SearchByProjection(const ResidentFrame& CurrentFrame, FrameData& members,
                                   const ProjectedLastFrame& LastFrame, const float th, const bool bMono,
                                   std::vector<int>& vpMapPointMatches) {
    FrameData F = with_resident(members, CurrentFrame);
    return SearchByProjection(F, LastFrame, th, bMono, vpMapPointMatches);
}

int ORBmatcher::SearchByProjection(const ResidentFrame& Fr, FrameData& members, const ProjectedMapPoints& vpMapPoints,
                                   const float th, std::vector<int>& vpMapPointMatches) {
    FrameData F = with_resident(members, Fr);
    return SearchByProjection(F, vpMapPoints, th, vpMapPointMatches);
}

int ORBmatcher::SearchByProjectionBird(const ResidentFrame& Fr, FrameData& members,
                                       const ProjectedBirdPoints& vpMapPointsBird, const float r,
                                       std::vector<int>& vpMapPointMatchesBird) {
    FrameData F = with_resident(members, Fr);
    return SearchByProjectionBird(F, vpMapPointsBird, r, vpMapPointMatchesBird);
}

int ORBmatcher::SearchByMatchBird(const KeyFrameBirdPoints& KF, const ResidentFrame& Fr,
                                  std::vector<int>& vpMapPointMatchesBird, const float r) {
    FrameData F = with_resident(FrameData(), Fr);
    return SearchByMatchBird(KF, F, vpMapPointMatchesBird, r);
}

int ORBmatcher::BirdviewMatch(const FrameData& F1, const ResidentFrame& F2, std::vector<int>& vnMatches12,
                              int windowSize) {
    return window_match(false, F1, with_resident(FrameData(), F2), nullptr, windowSize, vnMatches12);
}

/* ---------------- the searches over ResidentPoints: projection and search in one GPU call ---------------- */

int ORBmatcher::SearchLocalPoints(const ResidentPoints& points, const orb_camera& camera, const std::vector<int>& ids,
                                  const ResidentFrame& F, const FrameData& members, const float th,
                                  const float viewingCosLimit, std::vector<int>& vpMapPointMatches,
                                  std::vector<orb_point_proj>* proj) {
    require(points && F, "SearchLocalPoints: empty handle");
    const int n = (int)ids.size();
    vpMapPointMatches.assign(std::max(F.N(), 1), -1);
    if (proj) proj->assign(std::max(n, 1), orb_point_proj());
    int nmatches = 0;
    check(orb_search_local_points(matcher_ctx(), points.handle(), &camera, viewingCosLimit, th, mfNNratio, n,
                                  n ? ids.data() : nullptr, F.handle(), members.hasMapPoint, F.hasURight() ? 1 : 0,
                                  vpMapPointMatches.data(), &nmatches, proj ? proj->data() : nullptr),
          "SearchLocalPoints");
    vpMapPointMatches.resize(F.N());
    if (proj) proj->resize(n);
    return nmatches;
}

void ORBmatcher::FuseSearch(const ResidentPoints& points, const std::vector<FusePointsTarget>& targets,
                            std::vector<std::vector<FuseBest> >& best,
                            std::vector<std::vector<orb_point_proj> >* proj) {
    require((bool)points, "FuseSearch: empty points handle");
    const size_t nt = targets.size();
    std::vector<orb_fuse_points_target> T(std::max<size_t>(nt, 1));
    std::vector<std::vector<int> > idx(nt), dist(nt);
    if (proj) proj->assign(nt, std::vector<orb_point_proj>());
    for (size_t t = 0; t < nt; t++) {
        const FusePointsTarget& S = targets[t];
        require(S.kf && *S.kf, "FuseSearch: a target without its ResidentFrame");
        const size_t n = S.ids.size();
        idx[t].assign(std::max<size_t>(n, 1), -1);
        dist[t].assign(std::max<size_t>(n, 1), -1);
        if (proj) (*proj)[t].assign(std::max<size_t>(n, 1), orb_point_proj());
        T[t].camera = S.camera;
        T[t].frame = S.kf->handle();
        T[t].inv_sigma2 = S.invLevelSigma2;
        T[t].th = S.th;
        T[t].n = (int)n;
        T[t].ids = n ? S.ids.data() : nullptr;
        T[t].best_idx = idx[t].data();
        T[t].best_dist = dist[t].data();
        T[t].proj_out = proj ? (*proj)[t].data() : nullptr;
    }
    check(orb_fuse_search_points(matcher_ctx(), points.handle(), (int)nt, T.data()), "FuseSearch(ResidentPoints)");
    best.assign(nt, std::vector<FuseBest>());
    for (size_t t = 0; t < nt; t++) {
        const size_t n = targets[t].ids.size();
        best[t].resize(n);
        for (size_t i = 0; i < n; i++) best[t][i] = FuseBest{idx[t][i], dist[t][i]};
        if (proj) (*proj)[t].resize(n);
    }
}

std::vector<int> ComputeDistinctiveDescriptors(const std::vector<std::vector<const uint8_t*> >& observations) {
    const int nmp = (int)observations.size();
    std::vector<int> off(nmp + 1, 0), best(std::max(nmp, 1), -1);
    for (int m = 0; m < nmp; m++) off[m + 1] = off[m] + (int)observations[m].size();
    std::vector<uint8_t> flat((size_t)std::max(off[nmp], 1) * 32);
    for (int m = 0; m < nmp; m++)
        for (size_t j = 0; j < observations[m].size(); j++)
            memcpy(&flat[((size_t)off[m] + j) * 32], observations[m][j], 32);
    check(orb_distinctive_descriptors(matcher_ctx(), nmp, off.data(), flat.data(), best.data()),
          "ComputeDistinctiveDescriptors");
    best.resize(nmp);
    return best;
}

}  // namespace ORBGPU_MATCHER_NAMESPACE
