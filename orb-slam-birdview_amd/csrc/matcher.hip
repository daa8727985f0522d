// ORBmatcher entry points of the C-ABI.  Distances and top-k lists come from the gfx950 kernels
// (hamming_kernels.hip); the parts of the reference that depend on the ORDER of earlier accepted
// matches — SearchByBoW's "already assigned" skip (ORBmatcher.cc:209-210, :576/:603) and
// SearchForInitialization's vMatchedDistance stealing (:444-445, :463-470) — are replayed on the
// host in the reference's iteration order.  A top-k list is exact for a query as long as two of its
// entries are still admissible at replay time or it holds every admissible candidate; otherwise the
// remaining queries are re-ranked on the GPU against the current exclusion state.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "grid_window.h"
#include "orbgpu_ctx.h"
#include "point_project.h"
#include "topk_scan.h"
#include "tri_geometry.h"

namespace orbgpu {

// A FeatureVector CSR the walks below can trust: offsets start at 0 and never decrease (so the features of the
// nodes a walk visits number at most offsets[nnodes], the size the staging is allocated for), every feature index
// lies in [0, n) (the walks index the descriptors, keypoints and map-point flags with it), and node ids ascend
// strictly (for_common_nodes is the std::map merge, which assumes ordered unique keys).  O(nnodes + nnz).
bool featvec_ok(const orb_featvec& v, int n) {
    if (v.nnodes < 0 || (v.nnodes > 0 && (!v.offsets || !v.indices || !v.node_ids))) return false;
    if (v.nnodes == 0) return true;
    if (v.offsets[0] != 0) return false;
    for (int i = 0; i < v.nnodes; i++) {
        if (v.offsets[i + 1] < v.offsets[i]) return false;
        if (i > 0 && v.node_ids[i] <= v.node_ids[i - 1]) return false;
    }
    for (int k = 0; k < v.offsets[v.nnodes]; k++)
        if (v.indices[k] < 0 || v.indices[k] >= n) return false;
    return true;
}

namespace {

constexpr int TH_LOW = 50;          // ORBmatcher.cc:38
constexpr int TH_HIGH = 100;        // :37
constexpr int HISTO_LENGTH = 30;    // :39
constexpr int K = 8;

int rot_bin(float a1, float a2) {   // ORBmatcher.cc:236-243 (round(rot*(1/30)): bins 0..12, upstream quirk)
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = a1 - a2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)std::round(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

void three_maxima(const std::vector<int>* histo, int& ind1, int& ind2, int& ind3) {   // :1601-1642
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            ind3 = ind2; ind2 = i;
        } else if (s > max3) {
            max3 = s; ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

// Drop matches outside the three dominant rotation bins (e.g. :265-285).
void cull_rotation(const std::vector<int>* rotHist, std::vector<int>& matches, int& nmatches) {
    int i1 = -1, i2 = -1, i3 = -1;
    three_maxima(rotHist, i1, i2, i3);
    for (int i = 0; i < HISTO_LENGTH; i++) {
        if (i == i1 || i == i2 || i == i3) continue;
        for (int q : rotHist[i])
            if (matches[q] >= 0) { matches[q] = -1; nmatches--; }
    }
}

// The same cull where the reference has no ">= 0" guard (SearchForTriangulation :792-813, SearchByProjection
// :1448-1467, SearchByMatchBird :2093-2111): every entry of a culled bin resets its slot to reset_value and
// decrements the count, so a slot the histogram holds twice counts twice.
void cull_rotation_all(const std::vector<int>* rotHist, std::vector<int>& matches, int& nmatches, int reset_value) {
    int i1 = -1, i2 = -1, i3 = -1;
    three_maxima(rotHist, i1, i2, i3);
    for (int i = 0; i < HISTO_LENGTH; i++) {
        if (i == i1 || i == i2 || i == i3) continue;
        for (int q : rotHist[i]) { matches[q] = reset_value; nmatches--; }
    }
}

template <class F>
void for_common_nodes(const orb_featvec& a, const orb_featvec& b, F f) {   // std::map merge (:175-264)
    int i = 0, j = 0;
    while (i < a.nnodes && j < b.nnodes) {
        if (a.node_ids[i] == b.node_ids[j]) { f(i, j); i++; j++; }
        else if (a.node_ids[i] < b.node_ids[j]) i++;
        else j++;
    }
}

// What is wrong with a Frame grid CSR over nt trains, or NULL: cell_off missing, or cell_idx missing where the grid
// has slots; then the CSR itself, since the grid kernels read cell_idx[cell_off[..]] for every rectangle column and
// index the trains by cell_idx, so a malformed one would be an out-of-bounds device read.
const char* grid_csr_fault(const orb_frame_grid& g, int nt) {
    if (!g.cell_off || (g.cell_off[kFrameGridCells] && !g.cell_idx)) return "bad arguments";
    if (g.cell_off[0] != 0) return "grid cell_off[0] != 0";
    for (int i = 0; i < kFrameGridCells; i++)   // offsets non-decreasing, so every run lies in [0, cell_off[3072])
        if (g.cell_off[i + 1] < g.cell_off[i]) return "grid cell_off decreases";
    for (int i = 0, nslots = g.cell_off[kFrameGridCells]; i < nslots; i++)   // the device indexes the trains by these
        if (g.cell_idx[i] < 0 || g.cell_idx[i] >= nt) return "grid index out of range";
    return nullptr;
}

// The train side of a grid search: host arrays with their Frame grid CSR, staged and uploaded by the call, or a
// resident frame, whose arrays and grid are on the device already.  Either way n trains, the host keypoints the
// replays read, and the grid's geometry.
struct TrainSide {
    int n = 0;
    const orb_keypoint* kps = nullptr;
    float min_x = 0, min_y = 0, inv_w = 0, inv_h = 0;
    const uint8_t* desc = nullptr;   // the host form: descriptors, uright (NULL: no stereo gate), the grid's CSR
    const float* uright = nullptr;
    const int* cell_off = nullptr;
    const int* cell_idx = nullptr;
    const orb_frame* F = nullptr;    // the resident form (use_ur: gate on its uright)
    bool use_ur = false;

    TrainSide() = default;
    TrainSide(int nt, const uint8_t* tdesc, const orb_keypoint* kps_t, const float* t_uright, const orb_frame_grid& g)
        : n(nt), kps(kps_t), min_x(g.min_x), min_y(g.min_y), inv_w(g.inv_w), inv_h(g.inv_h), desc(tdesc),
          uright(t_uright), cell_off(g.cell_off), cell_idx(g.cell_idx) {}
    TrainSide(const orb_frame* frame, bool use_uright)   // (frame != NULL)
        : n(frame->n), kps(frame->kps.data()), min_x(frame->min_x), min_y(frame->min_y), inv_w(frame->inv_w),
          inv_h(frame->inv_h), F(frame), use_ur(use_uright) {}

    bool has_ur() const { return F ? use_ur : uright != nullptr; }
    // What is wrong with the host form (n >= 0), or NULL: an array missing, then the grid.  A resident frame's arrays
    // and CSR are the library's own
    const char* fault() const {
        if (F) return nullptr;
        if (n > 0 && (!desc || !kps)) return "bad arguments";
        return grid_csr_fault(orb_frame_grid{min_x, min_y, inv_w, inv_h, cell_off, cell_idx}, n);
    }
    bool on_other_device(const Ctx* c) const { return F && F->device != c->device; }
};

// A train side's place in a call's staging area.  The host form's regions are laid out in the kernels' order, [t | k2
// | ur] with add_arrays() and [cell_off | cell_idx] with add_grid(), and written with put(); a resident side has no
// regions and all three do nothing.  row() gives the device pointers the kernels take, into the staging area or into
// the frame's allocation, as a row of k_projection_best's table (inv_sigma2 left to the caller).
struct TrainStage {
    TrainSide s;
    bool ur = false;   // the kernel gates on uright
    size_t o_t = 0, o_k2 = 0, o_ur = 0, o_coff = 0, o_cidx = 0;
    size_t nslots() const { return (size_t)s.cell_off[kFrameGridCells]; }
    // ur_region: the layout has a uright region even without the gate (an empty one)
    void add_arrays(Stage& st, bool ur_region) {
        if (s.F) return;
        o_t = st.add((size_t)s.n * 32);
        o_k2 = st.add((size_t)s.n * sizeof(orb_keypoint));
        if (ur || ur_region) o_ur = st.add(ur ? (size_t)s.n * 4 : 0);
    }
    void add_grid(Stage& st) {
        if (s.F) return;
        o_coff = st.add((size_t)(kFrameGridCells + 1) * 4);
        o_cidx = st.add(nslots() * 4);
    }
    void put(const Stage& st) const {
        if (s.F) return;
        st.put(o_t, s.desc, (size_t)s.n * 32);
        st.put(o_k2, s.kps, (size_t)s.n * sizeof(orb_keypoint));
        if (ur) st.put(o_ur, s.uright, (size_t)s.n * 4);
        st.put(o_coff, s.cell_off, (size_t)(kFrameGridCells + 1) * 4);
        st.put(o_cidx, s.cell_idx, nslots() * 4);
    }
    ProjTarget row(const Stage& st) const {
        const ProjGrid g{s.min_x, s.min_y, s.inv_w, s.inv_h};
        if (const orb_frame* F = s.F)
            return ProjTarget{F->d_desc, F->d_kps, ur ? F->d_ur : nullptr, nullptr, F->d_coff, F->d_cidx, g};
        return ProjTarget{st.di<uint8_t>(o_t), st.di<orb_keypoint>(o_k2), ur ? st.di<float>(o_ur) : nullptr, nullptr,
                          st.di<int>(o_coff), st.di<int>(o_cidx), g};
    }
};

// One matcher call: static data on the device, re-rankable from any item with fresh thresholds.
struct TopkSession {
    // which ranking kernel the session drives, and so which input regions its arena holds before the common tail
    enum Mode {
        LIST,   // k_topk: inputs [q | t | rng | cand]
        GRID,   // k_window_topk (orb_window_match_grid): [q | item | cen | k1 | t | k2 | cell_off | cell_idx]
        PROJ    // k_projection_topk (orb_search_by_projection): [pq | q | t | k2 | ur | cell_off | cell_idx]
    };
    Ctx* c;
    int nitems = 0, nt = 0;
    std::vector<int> item_q;         // query feature per item
    std::vector<int2> item_rng;      // [begin, end) into cand
    // batch calls: the query row of each item (else qdesc + 32 item_q[i]) and the train set as consecutive parts
    // (else tdesc): several keyframes' items / trains in one session
    std::vector<const uint8_t*> item_src;
    std::vector<std::pair<const uint8_t*, int> > tparts;
    const int* cand = nullptr;       // host candidate list
    int ncand = 0;
    Stage st{c};
    Mode mode = LIST;
    // arena offsets: the mode's inputs, then the tail every mode shares: [thr] (o_in_end: the end of the uploaded
    // span) and the outputs [dist | idx | nvalid]
    size_t o_q = 0, o_t = 0, o_rng = 0, o_cand = 0, o_item = 0, o_cen = 0, o_k1 = 0, o_pq = 0;
    size_t o_thr = 0, o_in_end = 0, o_dist = 0, o_idx = 0, o_nv = 0;
    bool uploaded = false;
    // GRID / PROJ: the train side and its regions [t | k2 | ur | cell_off | cell_idx] (ur in PROJ only; none of them
    // for a resident frame, whose device pointers the launch takes)
    TrainStage train;
    float win_r = 0;       // GRID: the window's radius
    bool cen = false;      // GRID: window centres given (else kps1)
    int lanes = 64;        // PROJ: lanes per query
    // host results (indexed by item), in the pinned mirror
    const int* dist = nullptr;
    const int* idx = nullptr;
    const int* nvalid = nullptr;

    // The layout of a call: begin(), the mode's input regions in the kernel's order with st.add() (the train side's
    // with train.add_arrays() and train.add_grid()), finish_layout(), which appends the shared tail and allocates,
    // then the inputs with st.put() (train.put()) in that same order: the upload starts at offset 0, with the lines
    // written first.
    // begin() returns false when there is nothing to rank: no GPU work at all
    bool begin(Mode m, int n_items, int ntrain) {
        mode = m;
        nitems = n_items;
        nt = ntrain;
        st.c = c;
        return nitems > 0;
    }
    // device_queries: the queries and their descriptors are written on the device (setup_points): their regions come
    // last, past the end of the pinned mirror
    // resident_kfs > 0: the items are written on the device (setup_bow_frames): item_q and the segment lengths come
    // down in the mirror beside the lists, the item-major queries and the ranges are device-only regions
    int finish_layout(bool device_queries = false, int resident_kfs = 0) {
        o_thr = st.add((size_t)nt * 4);
        o_in_end = st.off;
        o_dist = st.add((size_t)nitems * K * 4);
        o_idx = st.add((size_t)nitems * K * 4);
        o_nv = st.add((size_t)nitems * 4);
        if (resident_kfs > 0) {
            o_itemq = st.add((size_t)nitems * 4);
            o_seglen = st.add((size_t)resident_kfs * 4);
            st.end_mirror();
            o_q = st.add((size_t)nitems * 32);
            o_rng = st.add((size_t)nitems * 8);
        }
        if (device_queries) {
            st.end_mirror();
            o_pq = st.add((size_t)nitems * sizeof(orb_proj_query));
            o_q = st.add((size_t)nitems * 32);
        }
        const int r = st.alloc();
        if (r != ORB_OK) return r;
        dist = st.h<int>(o_dist);
        idx = st.h<int>(o_idx);
        nvalid = st.h<int>(o_nv);
        return ORB_OK;
    }

    // List mode: item i = query item_q[i] (or the row item_src[i]) against the candidates cand[item_rng[i]].
    int setup(const uint8_t* qdesc, const uint8_t* tdesc, int ntrain) {
        if (!begin(LIST, (int)item_q.size(), ntrain)) return ORB_OK;
        o_q = st.add((size_t)nitems * 32);
        o_t = st.add((size_t)nt * 32);
        o_rng = st.add((size_t)nitems * 8);
        o_cand = st.add((size_t)ncand * 4);
        const int r = finish_layout();
        if (r != ORB_OK) return r;
        uint8_t* hq = st.hi<uint8_t>(o_q);
        for (int i = 0; i < nitems; i++)
            std::memcpy(hq + (size_t)i * 32, item_src.empty() ? qdesc + (size_t)item_q[i] * 32 : item_src[i], 32);
        if (tparts.empty()) st.put(o_t, tdesc, (size_t)nt * 32);
        size_t o = o_t;
        for (const auto& tp : tparts) {
            st.put(o, tp.first, (size_t)tp.second * 32);
            o += (size_t)tp.second * 32;
        }
        st.put(o_rng, item_rng.data(), (size_t)nitems * 8);
        st.put(o_cand, cand, (size_t)ncand * 4);
        return ORB_OK;
    }

    // Grid mode: queries = desc1 rows item_q[i] (uploaded whole, indexed on the device), candidates from
    // the window of radius r around centres[item_q[i]] (NULL: kps1) in the train side's grid.
    int setup_grid(const uint8_t* desc1, int n1, const orb_keypoint* kps1, const float* centres, float r,
                   const TrainSide& side) {
        if (!begin(GRID, (int)item_q.size(), side.n)) return ORB_OK;
        train = TrainStage{side, false};
        win_r = r;
        cen = centres != nullptr;
        const size_t kp1 = (size_t)n1 * sizeof(orb_keypoint);
        o_q = st.add((size_t)n1 * 32);
        o_item = st.add((size_t)nitems * 4);
        o_cen = st.add(cen ? (size_t)n1 * 8 : 0);
        o_k1 = st.add(kp1);
        train.add_arrays(st, false);
        train.add_grid(st);
        const int rr = finish_layout();
        if (rr != ORB_OK) return rr;
        st.put(o_q, desc1, (size_t)n1 * 32);
        st.put(o_item, item_q.data(), (size_t)nitems * 4);
        if (cen) st.put(o_cen, centres, (size_t)n1 * 8);
        st.put(o_k1, kps1, kp1);
        train.put(st);
        return ORB_OK;
    }

    // Projection mode (orb_search_by_projection): item i = query i with its own window (orb_proj_query) in the
    // train side's grid, with the stereo gate if the side has uright.
    int setup_proj(int nq, const orb_proj_query* q, const uint8_t* qdesc, const TrainSide& side, int nlanes) {
        if (!begin(PROJ, nq, side.n)) return ORB_OK;
        train = TrainStage{side, side.has_ur()};
        lanes = nlanes;
        const size_t pq = (size_t)nq * sizeof(orb_proj_query);
        o_pq = st.add(pq);
        o_q = st.add((size_t)nq * 32);
        train.add_arrays(st, true);
        train.add_grid(st);
        const int rr = finish_layout();
        if (rr != ORB_OK) return rr;
        st.put(o_pq, q, pq);
        st.put(o_q, qdesc, (size_t)nq * 32);
        train.put(st);
        return ORB_OK;
    }

    // Projection mode over resident map points (orb_search_local_points): item i = slot ids[i] of P projected through
    // cam (ORB_FRUSTUM_FRAME).  Only [camera | ids] are staged and go up; the queries and their descriptors are
    // device-only regions (past the mirror's end) that k_project_points fills, queued here ahead of the ranking, so
    // run() uploads nothing but its thresholds.  The kernel stores the records (want_rec) into the pinned mirror at o_rec.
    size_t o_cam = 0, o_ids = 0, o_rec = 0;
    int setup_points(const orb_points* P, const PointCam& cam, int n, const int* ids, const TrainSide& side,
                     int nlanes, bool want_rec) {
        if (!begin(PROJ, n, side.n)) return ORB_OK;
        train = TrainStage{side, side.has_ur()};
        lanes = nlanes;
        o_cam = st.add(sizeof(PointCam));
        o_ids = st.add((size_t)n * 4);
        const size_t in_end = st.off;
        o_rec = st.add(want_rec ? (size_t)n * sizeof(orb_point_proj) : 0);
        train.add_arrays(st, true);
        train.add_grid(st);
        const int rr = finish_layout(true);
        if (rr != ORB_OK) return rr;
        *st.hi<PointCam>(o_cam) = cam;
        st.put(o_ids, ids, (size_t)n * 4);
        train.put(st);
        hipError_t e;
        if ((e = st.up(0, in_end)) != hipSuccess) return set_error("upload", e), ORB_ERR_HIP;
        if ((e = launch_project_points(ORB_FRUSTUM_FRAME, st.d<PointCam>(o_cam), nullptr, st.d<int>(o_ids), n, P->d_geo,
                                       P->d_desc, want_rec ? st.h<orb_point_proj>(o_rec) : nullptr,
                                       st.d<orb_proj_query>(o_pq), st.d<uint8_t>(o_q), c->stream)) != hipSuccess)
            return set_error("k_project_points", e), ORB_ERR_HIP;
        uploaded = true;
        return ORB_OK;
    }

    // List mode between resident frames (orb_search_by_bow_frames_*): keyframe p's queries are the features of
    // kfs[p].q's FeatureVector that share a node with `train`'s and whose flag is set, its items the segment
    // [seg0_p, seg0_p + nnz_p) of the session (seg0_p = the earlier keyframes' CSR lengths), of which k_bow_items,
    // queued here, fills the first seg_len[p].  The trains and the candidate list are the train frame's descriptors
    // and its FeatureVector's indices: only [table | flags] go up.  fetch_items() after the first run() brings
    // item_q and each keyframe's [first, last) to the host.
    struct BowFrameKf {
        const orb_frame* q;
        const uint8_t* flag;
    };
    const uint8_t* r_t = nullptr;
    const int* r_cand = nullptr;
    size_t o_itemq = 0, o_seglen = 0;
    std::vector<int> seg0;
    int setup_bow_frames(int nkf, const BowFrameKf* kfs, const orb_frame* train) {
        long long cap = 0;
        seg0.assign(nkf + 1, 0);
        for (int p = 0; p < nkf; p++) seg0[p + 1] = (int)(cap += kfs[p].q->bow->nnz);
        if (cap > INT_MAX / 64) return arg_error("orb_search_by_bow_frames", "too many features");
        if (!begin(LIST, (int)cap, train->n)) return ORB_OK;
        const size_t o_tab = st.add((size_t)nkf * sizeof(BowItemsRow));
        std::vector<size_t> o_flag(nkf);
        for (int p = 0; p < nkf; p++) o_flag[p] = st.add((size_t)kfs[p].q->n);
        const size_t in_end = st.off;
        const int r = finish_layout(false, nkf);
        if (r != ORB_OK) return r;
        const orb_frame_bow* T = train->bow;
        BowItemsRow* tab = st.hi<BowItemsRow>(o_tab);
        for (int p = 0; p < nkf; p++) {
            const orb_frame* Q = kfs[p].q;
            const orb_frame_bow* B = Q->bow;
            st.put(o_flag[p], kfs[p].flag, (size_t)Q->n);
            tab[p] = BowItemsRow{B->d<uint32_t>(B->L.o_nodes), B->d<int>(B->L.o_off), B->d<int>(B->L.o_idx), Q->d_desc,
                                 st.d<uint8_t>(o_flag[p]), T->d<uint32_t>(T->L.o_nodes), T->d<int>(T->L.o_off),
                                 B->nnodes, B->nnz, T->nnodes, seg0[p], 0, 0};
        }
        r_t = train->d_desc;
        r_cand = T->d<int>(T->L.o_idx);
        hipError_t e;
        if ((e = st.up(0, in_end)) != hipSuccess) return set_error("upload", e), ORB_ERR_HIP;
        if ((e = launch_bow_items(st.d<BowItemsRow>(o_tab), nkf, st.h<int>(o_itemq), st.d<int2>(o_rng),
                                  st.d<uint8_t>(o_q), st.h<int>(o_seglen), c->stream)) != hipSuccess)
            return set_error("k_bow_items", e), ORB_ERR_HIP;
        uploaded = true;
        return ORB_OK;
    }
    // keyframe p's live items [first[p], last[p]) and item_q, once run() has synchronised
    void fetch_items(std::vector<int>& first, std::vector<int>& last) {
        const int nkf = (int)seg0.size() - 1;
        first.assign(seg0.begin(), seg0.begin() + nkf);
        last = first;
        if (nitems <= 0) return;
        item_q.assign(st.h<int>(o_itemq), st.h<int>(o_itemq) + nitems);
        for (int p = 0; p < nkf; p++) last[p] = first[p] + std::min(st.h<int>(o_seglen)[p], seg0[p + 1] - seg0[p]);
    }

    // Rank items [from, to) (to < 0: nitems) with train thresholds thr (NULL = admit all).
    int run(int from, const int* thr, int to = -1) {
        const int n = (to < 0 ? nitems : to) - from;
        if (n <= 0) return ORB_OK;
        hipError_t e;
        if (thr) std::memcpy(st.hi<int>(o_thr), thr, (size_t)nt * 4);
        // first call: the whole input span in one DMA; a re-rank: the thresholds only
        if ((e = uploaded ? (thr ? st.up(o_thr, o_thr + (size_t)nt * 4) : hipSuccess) : st.up(0, o_in_end)) != hipSuccess)
            return set_error("upload", e), ORB_ERR_HIP;
        uploaded = true;
        const int* d_thr = thr ? st.di<int>(o_thr) : nullptr;
        // the kernel writes the lists straight into the pinned mirror (host-coherent memory; items before
        // `from` keep their values): no D2H command, one synchronisation
        int* const out_dist = st.h<int>(o_dist) + (size_t)from * K;
        int* const out_idx = st.h<int>(o_idx) + (size_t)from * K;
        int* const out_nv = st.h<int>(o_nv) + from;
        const ProjTarget T = train.row(st);   // GRID / PROJ: the train side, staged or resident
        if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 1, c->stream);
        switch (mode) {
        case PROJ:
            e = launch_projection_topk(st.di<orb_proj_query>(o_pq) + from, st.di<uint8_t>(o_q) + (size_t)from * 32, n,
                                       T.t, T.kps, T.ur, T.cell_off, T.cell_idx, T.g, d_thr, K, lanes, out_dist, out_idx,
                                       out_nv, c->stream);
            break;
        case GRID:
            e = launch_window_topk(st.di<uint8_t>(o_q), st.di<int>(o_item) + from, cen ? st.di<float2>(o_cen) : nullptr, n,
                                   st.di<orb_keypoint>(o_k1), T.t, T.kps, T.cell_off, T.cell_idx,
                                   WinGrid{T.g.min_x, T.g.min_y, T.g.inv_w, T.g.inv_h, win_r}, d_thr, K, out_dist, out_idx,
                                   out_nv, c->stream);
            break;
        case LIST:
            e = launch_hamming_topk(st.di<uint8_t>(o_q) + (size_t)from * 32, n, r_t ? r_t : st.di<uint8_t>(o_t), nt,
                                    st.di<int2>(o_rng) + from, r_cand ? r_cand : st.di<int>(o_cand), d_thr, K, out_dist,
                                    out_idx, out_nv, c->stream);
            break;
        }
        if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 0, c->stream);
        if (e != hipSuccess) return set_error("hamming kernel", e), ORB_ERR_HIP;
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess)
            return set_error("download top-k", e), ORB_ERR_HIP;
        return ORB_OK;
    }

    // The first `need` entries of item i's list that admit(train, distance) accepts (topk_scan.h).  A list that cannot
    // decide them is ranked again from item i on (to `to`) against the thresholds fill_thr() returns, which state
    // what the replay admits now, and scanned once more: the new list starts with the item's best admissible trains.
    template <class Admit, class FillThr>
    int pick(int i, int need, Admit admit, int stop_at, FillThr fill_thr, int to, TopkPick& p) {
        if (topk_scan(dist, idx, nvalid, K, i, need, admit, stop_at, p)) return ORB_OK;
        const int r = run(i, fill_thr(), to);
        if (r != ORB_OK) return r;
        topk_scan(dist, idx, nvalid, K, i, need, admit, stop_at, p);
        return ORB_OK;
    }
};

// SearchByBoW(KeyFrame*, Frame&)'s acceptance (ORBmatcher.cc:175-283) over one keyframe's items [ib, ie), in the
// reference's order: the first two admissible entries of each top-k list (a taken Frame feature is skipped), the
// ratio test, the rotation histogram; a list the taken set exhausts is re-ranked on the GPU from that item on.
// Trains are the Frame's features (indices 0..n_f).
int bow_kf_f_replay(TopkSession& s, int ib, int ie, float nnratio, int check_ori, int n_f, const float* angle_kf,
                    const float* angle_f, int* match_f, int* nmatches_out) {
    std::vector<int> matches(n_f, -1);
    std::vector<int> thr(n_f);
    std::vector<int> rotHist[HISTO_LENGTH];
    int nmatches = 0;
    auto admit = [&](int t, int) { return matches[t] < 0; };   // if(vpMapPointMatches[realIdxF]) continue;
    auto fill_thr = [&]() {
        for (int t = 0; t < n_f; t++) thr[t] = matches[t] >= 0 ? -1 : INT_MAX;
        return thr.data();
    };
    TopkPick p;
    for (int i = ib; i < ie; i++) {
        const int st = s.pick(i, 2, admit, kTopkNoStop, fill_thr, ie, p);
        if (st != ORB_OK) return st;
        const int d1 = p.dist(0, 256), i1 = p.t[0], d2 = p.dist(1, 256);   // bestDist1 = bestDist2 = 256 (:201-203)
        if (d1 <= TH_LOW && static_cast<float>(d1) < nnratio * static_cast<float>(d2)) {   // :228-230
            const int realIdxKF = s.item_q[i];
            matches[i1] = realIdxKF;
            if (check_ori) rotHist[rot_bin(angle_kf[realIdxKF], angle_f[i1])].push_back(i1);
            nmatches++;
        }
    }
    if (check_ori) cull_rotation(rotHist, matches, nmatches);
    std::memcpy(match_f, matches.data(), (size_t)n_f * sizeof(int));
    if (nmatches_out) *nmatches_out = nmatches;
    return ORB_OK;
}

// SearchByBoW(KeyFrame*, KeyFrame*)'s acceptance (:559-653) over one KF2's items [ib, ie); its trains are the
// session's train records [tb, tb + n2), thr the session-wide thresholds (this KF2's span rewritten on a re-rank).
int bow_kf_kf_replay(TopkSession& s, int ib, int ie, int tb, std::vector<int>& thr, float nnratio, int check_ori,
                     int n1, const float* angle1, int n2, const float* angle2, const uint8_t* mp2, int* match12,
                     int* nmatches_out) {
    std::vector<char> matched2(n2, 0);
    std::vector<int> matches(n1, -1);
    std::vector<int> rotHist[HISTO_LENGTH];
    int nmatches = 0;
    auto admit = [&](int t, int) { return !matched2[t - tb]; };   // if(vbMatched2[idx2] || !pMP2) continue; (:576-577)
    auto fill_thr = [&]() {
        for (int t = 0; t < n2; t++) thr[tb + t] = (matched2[t] || !mp2[t]) ? -1 : INT_MAX;
        return thr.data();
    };
    TopkPick p;
    for (int i = ib; i < ie; i++) {
        const int st = s.pick(i, 2, admit, kTopkNoStop, fill_thr, ie, p);
        if (st != ORB_OK) return st;
        const int d1 = p.dist(0, 256), i1 = p.t[0], d2 = p.dist(1, 256);   // bestDist1 = bestDist2 = 256 (:566-568)
        if (d1 < TH_LOW && static_cast<float>(d1) < nnratio * static_cast<float>(d2)) {   // :598-600
            const int idx1 = s.item_q[i], j2 = i1 - tb;
            matches[idx1] = j2;
            matched2[j2] = 1;
            if (check_ori) rotHist[rot_bin(angle1[idx1], angle2[j2])].push_back(idx1);
            nmatches++;
        }
    }
    if (check_ori) cull_rotation(rotHist, matches, nmatches);
    std::memcpy(match12, matches.data(), (size_t)n1 * sizeof(int));
    if (nmatches_out) *nmatches_out = nmatches;
    return ORB_OK;
}

bool bow_kf_ok(const orb_bow_kf& k) {
    return k.n >= 0 && k.match && featvec_ok(k.fv, k.n) && (k.n == 0 || (k.desc && k.angle && k.mp));
}

// SearchByBoW(KeyFrame*, Frame&) for nkf keyframes against one Frame: every keyframe's items in one session (the
// Frame's features are the shared trains and its FeatureVector the shared candidate list), one ranking launch, then
// each keyframe's replay.  The single call is the batch of one.
int bow_kf_f_run(Ctx* c, float nnratio, int check_ori, int n_f, const uint8_t* desc_f, const float* angle_f,
                 orb_featvec fv_f, int nkf, const orb_bow_kf* kfs) {
    TopkSession s{c};
    s.cand = fv_f.indices;
    s.ncand = fv_f.nnodes ? fv_f.offsets[fv_f.nnodes] : 0;
    std::vector<int> first(nkf + 1, 0);
    for (int p = 0; p < nkf; p++) {
        const orb_bow_kf& K = kfs[p];
        for_common_nodes(K.fv, fv_f, [&](int a, int b) {
            for (int iKF = K.fv.offsets[a]; iKF < K.fv.offsets[a + 1]; iKF++) {
                const int realIdxKF = K.fv.indices[iKF];
                if (!K.mp[realIdxKF]) continue;   // !pMP || pMP->isBad()  (:204-208)
                s.item_q.push_back(realIdxKF);
                s.item_src.push_back(K.desc + (size_t)realIdxKF * 32);
                s.item_rng.push_back(make_int2(fv_f.offsets[b], fv_f.offsets[b + 1]));
            }
        });
        first[p + 1] = (int)s.item_q.size();
    }
    int st = s.setup(nullptr, desc_f, n_f);
    if (st == ORB_OK) st = s.run(0, nullptr);
    if (st != ORB_OK) return st;
    for (int p = 0; p < nkf && st == ORB_OK; p++)
        st = bow_kf_f_replay(s, first[p], first[p + 1], nnratio, check_ori, n_f, kfs[p].angle, angle_f, kfs[p].match,
                             kfs[p].nmatches);
    return st;
}

// SearchByBoW(KeyFrame*, KeyFrame*) for one KF1 against nkf KF2s: the KF2s' features concatenated as the trains
// (KF2 p at [tb_p, tb_p + n2_p)), their FeatureVector indices concatenated (offset by tb_p) as the candidates.
int bow_kf_kf_run(Ctx* c, float nnratio, int check_ori, int n1, const uint8_t* desc1, const float* angle1,
                  const uint8_t* mp1, orb_featvec fv1, int nkf, const orb_bow_kf* kf2s) {
    TopkSession s{c};
    std::vector<int> first(nkf + 1, 0), tb(nkf + 1, 0), cand;
    std::vector<int> thr;
    for (int p = 0; p < nkf; p++) {
        const orb_bow_kf& K = kf2s[p];
        const int cb = (int)cand.size();
        const int nnz = K.fv.nnodes ? K.fv.offsets[K.fv.nnodes] : 0;
        for (int i = 0; i < nnz; i++) cand.push_back(tb[p] + K.fv.indices[i]);
        for_common_nodes(fv1, K.fv, [&](int a, int b) {
            for (int i = fv1.offsets[a]; i < fv1.offsets[a + 1]; i++) {
                const int idx1 = fv1.indices[i];
                if (!mp1[idx1]) continue;   // :567-571
                s.item_q.push_back(idx1);
                s.item_rng.push_back(make_int2(cb + K.fv.offsets[b], cb + K.fv.offsets[b + 1]));
            }
        });
        first[p + 1] = (int)s.item_q.size();
        tb[p + 1] = tb[p] + K.n;
        s.tparts.push_back(std::make_pair(K.desc, K.n));
        for (int t = 0; t < K.n; t++) thr.push_back(K.mp[t] ? INT_MAX : -1);   // !pMP2 || isBad (:584-588)
    }
    s.cand = cand.data();
    s.ncand = (int)cand.size();
    int st = s.setup(desc1, nullptr, tb[nkf]);
    if (st == ORB_OK) st = s.run(0, thr.data());
    if (st != ORB_OK) return st;
    for (int p = 0; p < nkf && st == ORB_OK; p++)
        st = bow_kf_kf_replay(s, first[p], first[p + 1], tb[p], thr, nnratio, check_ori, n1, angle1, kf2s[p].n,
                              kf2s[p].angle, kf2s[p].mp, kf2s[p].match, kf2s[p].nmatches);
    return st;
}

// The BoW searches between resident frames: the items come from k_bow_items, the lists from k_topk over the train
// frame's own arrays, the acceptance from the replays above, with the angles of the handles' host keypoints.
std::vector<float> frame_angles(const orb_frame* F) {
    std::vector<float> a((size_t)F->n);
    for (int i = 0; i < F->n; i++) a[i] = F->kps[i].angle;
    return a;
}

int bow_frames_kf_f_run(Ctx* c, float nnratio, int check_ori, const orb_frame* Ff, int nkf, const orb_bow_frame_kf* kfs) {
    TopkSession s{c};
    std::vector<TopkSession::BowFrameKf> q(nkf);
    for (int p = 0; p < nkf; p++) q[p] = TopkSession::BowFrameKf{kfs[p].frame, kfs[p].mp};
    int st = s.setup_bow_frames(nkf, q.data(), Ff);
    if (st == ORB_OK) st = s.run(0, nullptr);
    if (st != ORB_OK) return st;
    std::vector<int> first, last;
    s.fetch_items(first, last);
    const std::vector<float> angle_f = frame_angles(Ff);
    for (int p = 0; p < nkf && st == ORB_OK; p++)
        st = bow_kf_f_replay(s, first[p], last[p], nnratio, check_ori, Ff->n, frame_angles(kfs[p].frame).data(),
                             angle_f.data(), kfs[p].match, kfs[p].nmatches);
    return st;
}

int bow_frames_kf_kf_run(Ctx* c, float nnratio, int check_ori, const orb_frame* F1, const uint8_t* mp1,
                         const orb_frame* F2, const uint8_t* mp2, int* match12, int* nmatches) {
    TopkSession s{c};
    const TopkSession::BowFrameKf q{F1, mp1};
    std::vector<int> thr((size_t)F2->n);
    for (int t = 0; t < F2->n; t++) thr[t] = mp2[t] ? INT_MAX : -1;   // !pMP2 || isBad (:584-588)
    int st = s.setup_bow_frames(1, &q, F2);
    if (st == ORB_OK) st = s.run(0, thr.data());
    if (st != ORB_OK) return st;
    std::vector<int> first, last;
    s.fetch_items(first, last);
    return bow_kf_kf_replay(s, first[0], last[0], 0, thr, nnratio, check_ori, F1->n, frame_angles(F1).data(), F2->n,
                            frame_angles(F2).data(), mp2, match12, nmatches);
}

// What is wrong with a handle the vocabulary-gated searches take, or NULL
const char* bow_frame_fault(const orb_frame* F) {
    if (!F) return "NULL frame";
    if (!F->bow) return "a frame carries no BoW";
    return nullptr;
}

}  // namespace
}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_descriptor_distance(const uint8_t* a, const uint8_t* b) {   // ORBmatcher.cc:1647-1663
    int d = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * i, 4);
        std::memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

int orb_hamming_top2_slices(int npairs, int max_nq, int max_nt) {
    return orbgpu::top2_launch_slices(npairs, max_nq, max_nt);
}

int orb_hamming_top2_mfma_bits(void) { return 4; }   // the e2m1 form is the only one (hamming_top2.hip)

int orb_hamming_topk(orb_ctx* h, const uint8_t* q, int nq, const uint8_t* t, int nt, const int* cand_off,
                     const int* cand_idx, const int* train_thr, int k, int* out_dist, int* out_idx, int* out_nvalid) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (nq < 0 || nt < 0 || k < 1 || k > K || (nq && (!q || !out_dist || !out_idx)) || (nt && !t))
        return set_error("orb_hamming_topk: bad arguments", hipSuccess), ORB_ERR_ARG;
    if (nq == 0) return ORB_OK;
    const int ncand = cand_off ? cand_off[nq] : 0;
    Arena a{c};
    hipError_t e = a.reserve(Arena::align((size_t)nq * 32) + Arena::align((size_t)nt * 32) + Arena::align(nq * 8) +
                             Arena::align((size_t)ncand * 4) + Arena::align((size_t)nt * 4) +
                             2 * Arena::align((size_t)nq * k * 4) + Arena::align(nq * 4) + 4096);
    if (e != hipSuccess) return set_error("scratch", e), ORB_ERR_NOMEM;
    uint8_t* d_q = a.take<uint8_t>((size_t)nq * 32);
    uint8_t* d_t = a.take<uint8_t>((size_t)nt * 32);
    int2* d_rng = a.take<int2>(nq);
    int* d_cand = a.take<int>(ncand);
    int* d_thr = a.take<int>(nt);
    int* d_dist = a.take<int>((size_t)nq * k);
    int* d_idx = a.take<int>((size_t)nq * k);
    int* d_nv = a.take<int>(nq);
    std::vector<int2> rng;
    if (cand_off) {
        rng.resize(nq);
        for (int i = 0; i < nq; i++) rng[i] = make_int2(cand_off[i], cand_off[i + 1]);
    }
    if ((e = hipMemcpyAsync(d_q, q, (size_t)nq * 32, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (nt && (e = hipMemcpyAsync(d_t, t, (size_t)nt * 32, hipMemcpyHostToDevice, c->stream)) != hipSuccess) ||
        (cand_off && (e = hipMemcpyAsync(d_rng, rng.data(), nq * sizeof(int2), hipMemcpyHostToDevice, c->stream)) !=
                         hipSuccess) ||
        (ncand && (e = hipMemcpyAsync(d_cand, cand_idx, (size_t)ncand * 4, hipMemcpyHostToDevice, c->stream)) !=
                      hipSuccess) ||
        (train_thr && (e = hipMemcpyAsync(d_thr, train_thr, (size_t)nt * 4, hipMemcpyHostToDevice, c->stream)) !=
                          hipSuccess))
        return set_error("upload", e), ORB_ERR_HIP;
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 1, c->stream);
    e = launch_hamming_topk(d_q, nq, d_t, nt, cand_off ? d_rng : nullptr, d_cand, train_thr ? d_thr : nullptr, k,
                            d_dist, d_idx, d_nv, c->stream);
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 0, c->stream);
    if (e != hipSuccess) return set_error("hamming kernel", e), ORB_ERR_HIP;
    if ((e = hipMemcpyAsync(out_dist, d_dist, (size_t)nq * k * 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(out_idx, d_idx, (size_t)nq * k * 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (out_nvalid && (e = hipMemcpyAsync(out_nvalid, d_nv, (size_t)nq * 4, hipMemcpyDeviceToHost, c->stream)) !=
                           hipSuccess) ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return set_error("download", e), ORB_ERR_HIP;
    return ORB_OK;
}

int orb_hamming_top2_device(orb_ctx* h, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int* d_best,
                            int* d_best_idx, int* d_second) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (nq <= 0) return ORB_OK;
    if (nt > 65535) return set_error("orb_hamming_top2_device: more than 65535 trains", hipSuccess), ORB_ERR_ARG;
    Arena a{c};
    const int ns = top2_batch_slices(1, nq, nt);
    hipError_t e = a.reserve(Arena::align((size_t)ns * nq * sizeof(uint2)) + 512);
    if (e != hipSuccess) return set_error("scratch", e), ORB_ERR_NOMEM;
    uint2* part = a.take<uint2>((size_t)ns * nq);
    Top2Batch tb{d_q, d_t, 0, 0, nullptr, nq, nt, nullptr, 0, nq, 0, 0};
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 1, c->stream);
    e = launch_hamming_top2_batch(tb, 1, nq, nt, d_best, d_best_idx, d_second, part, c->stream);
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 0, c->stream);
    return e == hipSuccess ? ORB_OK : (set_error("top2 kernel", e), ORB_ERR_HIP);
}

int orb_hamming_top2_frames_device(orb_ctx* h, const uint8_t* d_desc, const int* d_counts, int kp_cap, int npairs,
                                   const int* q_frames, const int* t_frames, int* d_best, int* d_best_idx,
                                   int* d_second) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (npairs <= 0) return ORB_OK;
    if (!d_desc || !d_counts || kp_cap <= 0 || kp_cap > 65535 || !q_frames || !t_frames || !d_best ||
        !d_best_idx || !d_second)
        return set_error("orb_hamming_top2_frames_device: bad arguments", hipSuccess), ORB_ERR_ARG;
    for (int p = 0; p < npairs; p++)
        if (q_frames[p] < 0 || t_frames[p] < 0)
            return set_error("orb_hamming_top2_frames_device: negative frame index", hipSuccess), ORB_ERR_ARG;
    hipError_t e;
    // the pair list (q, t per pair) lives in its own device buffer and goes up only when it differs from the
    // previous call's: a caller that matches the same frame slots every batch (the bench, a tracking loop over a
    // ring of slots) pays no copy and no host wait per call.  A changed list is stream-ordered behind the launches
    // that still read the old one.
    bool same = (int)c->pairs_last.size() == 2 * npairs && c->d_pairs;
    for (int p = 0; p < npairs && same; p++)
        same = c->pairs_last[2 * p] == q_frames[p] && c->pairs_last[2 * p + 1] == t_frames[p];
    if (!same) {
        // the new list is committed to pairs_last only once its upload is queued: after any failure below the cache
        // still names what d_pairs holds (or is empty), so a retry with the same list uploads it again
        std::vector<int> want((size_t)2 * npairs);
        for (int p = 0; p < npairs; p++) {
            want[2 * p] = q_frames[p];
            want[2 * p + 1] = t_frames[p];
        }
        const size_t bytes = (size_t)npairs * sizeof(int2);
        constexpr size_t kPairsFloor = 4096 / sizeof(int2);
        if ((size_t)npairs > c->d_pairs.cap() || !c->d_pairs) {
            c->pairs_last.clear();   // d_pairs is about to be replaced: its old contents are no longer cached
            // (a launch queued earlier may still read the old buffer)
            if (c->d_pairs && (e = hipStreamSynchronize(c->stream)) != hipSuccess)
                return set_error("sync", e), ORB_ERR_HIP;
            if ((e = c->d_pairs.ensure(npairs, kPairsFloor)) != hipSuccess)
                return set_error("hipMalloc pairs", e), ORB_ERR_NOMEM;
        }
        // staged through two pinned slots used in turn: a slot is rewritten only after the event recorded behind
        // its previous upload has completed (the call returns before its copy runs)
        const int sl = c->pairs_slot;
        c->pairs_slot ^= 1;
        if (c->pairs_ev[sl] && (e = hipEventSynchronize(c->pairs_ev[sl])) != hipSuccess)
            return set_error("pairs staging event", e), ORB_ERR_HIP;
        if (!c->pairs_ev[sl] && (e = hipEventCreateWithFlags(&c->pairs_ev[sl], hipEventDisableTiming)) != hipSuccess)
            return set_error("pairs staging event", e), ORB_ERR_HIP;
        if ((e = c->h_pairs[sl].ensure(npairs, kPairsFloor)) != hipSuccess)
            return set_error("pairs pinned staging", e), ORB_ERR_NOMEM;
        std::memcpy(c->h_pairs[sl].get(), want.data(), bytes);
        if ((e = hipMemcpyAsync(c->d_pairs.get(), c->h_pairs[sl].get(), bytes, hipMemcpyHostToDevice, c->stream)) !=
                hipSuccess ||
            (e = hipEventRecord(c->pairs_ev[sl], c->stream)) != hipSuccess) {
            c->pairs_last.clear();   // the copy may or may not be queued: d_pairs' contents are unknown
            return set_error("upload pairs", e), ORB_ERR_HIP;
        }
        c->pairs_last.swap(want);
    }
    Arena a{c};
    const int ns = top2_batch_slices(npairs, kp_cap, kp_cap);
    if ((e = a.reserve(Arena::align((size_t)npairs * ns * kp_cap * sizeof(uint2)) + 512)) != hipSuccess)
        return set_error("scratch", e), ORB_ERR_NOMEM;
    uint2* part = a.take<uint2>((size_t)npairs * ns * kp_cap);
    Top2Batch tb{d_desc, d_desc, kp_cap, kp_cap, d_counts, 0, 0, c->d_pairs.get(), 0, kp_cap, 0, 0};
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 1, c->stream);
    e = launch_hamming_top2_batch(tb, npairs, kp_cap, kp_cap, d_best, d_best_idx, d_second, part, c->stream);
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 0, c->stream);
    return e == hipSuccess ? ORB_OK : (set_error("top2 kernel", e), ORB_ERR_HIP);
}

/* SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)  ORBmatcher.cc:159-288 */
int orb_search_by_bow_kf_f(orb_ctx* h, float nnratio, int check_ori, int n_kf, const uint8_t* desc_kf,
                           const float* angle_kf, const uint8_t* mp_kf, orb_featvec fv_kf, int n_f,
                           const uint8_t* desc_f, const float* angle_f, orb_featvec fv_f, int* match_f,
                           int* nmatches_out) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (n_kf < 0 || n_f < 0 || !match_f) return ORB_ERR_ARG;
    if (!featvec_ok(fv_kf, n_kf) || !featvec_ok(fv_f, n_f))
        return arg_error("orb_search_by_bow_kf_f", "malformed FeatureVector CSR");
    const orb_bow_kf K{n_kf, desc_kf, angle_kf, mp_kf, fv_kf, match_f, nmatches_out};
    return bow_kf_f_run(c, nnratio, check_ori, n_f, desc_f, angle_f, fv_f, 1, &K);
}

int orb_search_by_bow_kf_f_batch(orb_ctx* h, float nnratio, int check_ori, int n_f, const uint8_t* desc_f,
                                 const float* angle_f, orb_featvec fv_f, int nkf, const orb_bow_kf* kfs) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (n_f < 0 || nkf < 0 || (nkf > 0 && !kfs) || (n_f > 0 && !(desc_f && angle_f))) return ORB_ERR_ARG;
    if (!featvec_ok(fv_f, n_f)) return arg_error("orb_search_by_bow_kf_f_batch", "malformed FeatureVector CSR");
    for (int p = 0; p < nkf; p++)
        if (!bow_kf_ok(kfs[p])) return arg_error("orb_search_by_bow_kf_f_batch", "bad keyframe arguments");
    return nkf ? bow_kf_f_run(c, nnratio, check_ori, n_f, desc_f, angle_f, fv_f, nkf, kfs) : ORB_OK;
}

/* SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)  ORBmatcher.cc:522-655 */
int orb_search_by_bow_kf_kf(orb_ctx* h, float nnratio, int check_ori, int n1, const uint8_t* desc1,
                            const float* angle1, const uint8_t* mp1, orb_featvec fv1, int n2, const uint8_t* desc2,
                            const float* angle2, const uint8_t* mp2, orb_featvec fv2, int* match12,
                            int* nmatches_out) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (n1 < 0 || n2 < 0 || !match12) return ORB_ERR_ARG;
    if (!featvec_ok(fv1, n1) || !featvec_ok(fv2, n2))
        return arg_error("orb_search_by_bow_kf_kf", "malformed FeatureVector CSR");
    const orb_bow_kf K{n2, desc2, angle2, mp2, fv2, match12, nmatches_out};
    return bow_kf_kf_run(c, nnratio, check_ori, n1, desc1, angle1, mp1, fv1, 1, &K);
}

int orb_search_by_bow_kf_kf_batch(orb_ctx* h, float nnratio, int check_ori, int n1, const uint8_t* desc1,
                                  const float* angle1, const uint8_t* mp1, orb_featvec fv1, int nkf,
                                  const orb_bow_kf* kf2s) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (n1 < 0 || nkf < 0 || (nkf > 0 && !kf2s) || (n1 > 0 && !(desc1 && angle1 && mp1))) return ORB_ERR_ARG;
    if (!featvec_ok(fv1, n1)) return arg_error("orb_search_by_bow_kf_kf_batch", "malformed FeatureVector CSR");
    long long ntot = 0;
    for (int p = 0; p < nkf; p++) {
        if (!bow_kf_ok(kf2s[p])) return arg_error("orb_search_by_bow_kf_kf_batch", "bad keyframe arguments");
        ntot += kf2s[p].n;
    }
    if (ntot > INT_MAX / 64) return arg_error("orb_search_by_bow_kf_kf_batch", "too many features");
    return nkf ? bow_kf_kf_run(c, nnratio, check_ori, n1, desc1, angle1, mp1, fv1, nkf, kf2s) : ORB_OK;
}

int orb_search_by_bow_frames_kf_f(orb_ctx* h, float nnratio, int check_ori, const orb_frame* frame_f, int nkf,
                                  const orb_bow_frame_kf* kfs) {
    const char* const fn = "orb_search_by_bow_frames_kf_f";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (nkf < 0 || (nkf > 0 && !kfs)) return arg_error(fn, "bad arguments");
    if (const char* why = bow_frame_fault(frame_f)) return arg_error(fn, why);
    for (int p = 0; p < nkf; p++) {
        if (const char* why = bow_frame_fault(kfs[p].frame)) return arg_error(fn, why);
        if (kfs[p].frame->device != frame_f->device) return arg_error(fn, "frames of different devices");
        if (!kfs[p].match || (kfs[p].frame->n > 0 && !kfs[p].mp)) return arg_error(fn, "bad keyframe arguments");
    }
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    if (frame_f->device != c->device) return arg_error(fn, "frame of another device");
    CTX_GUARD(c);
    return nkf ? bow_frames_kf_f_run(c, nnratio, check_ori, frame_f, nkf, kfs) : ORB_OK;
}

int orb_search_by_bow_frames_kf_kf(orb_ctx* h, float nnratio, int check_ori, const orb_frame* kf1, const uint8_t* mp1,
                                   const orb_frame* kf2, const uint8_t* mp2, int* match12, int* nmatches) {
    const char* const fn = "orb_search_by_bow_frames_kf_kf";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const char* why = bow_frame_fault(kf1)) return arg_error(fn, why);
    if (const char* why = bow_frame_fault(kf2)) return arg_error(fn, why);
    if (!match12 || (kf1->n > 0 && !mp1) || (kf2->n > 0 && !mp2)) return arg_error(fn, "bad arguments");
    if (kf1->device != kf2->device) return arg_error(fn, "frames of different devices");
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    if (kf1->device != c->device) return arg_error(fn, "frame of another device");
    CTX_GUARD(c);
    return bow_frames_kf_kf_run(c, nnratio, check_ori, kf1, mp1, kf2, mp2, match12, nmatches);
}

/* SearchForTriangulation  ORBmatcher.cc:657-823: no cross-query dependence (vbMatched2 is never
 * set, :738), so every (idx1, node) item is decided on the GPU. */
}  // extern "C"

namespace orbgpu {
namespace {
// One keyframe pair's staging for k_triangulation, appended at the current ends of the item / train records:
// per common node its candidates without a map point (and stereo ones only if asked, :725-733) as train records in
// the node's order (the reference keeps the last candidate reaching the minimum), then one item record per query of
// the node that has candidates (a query with none matches nothing).  The pair-dependent float work follows in
// the reference build's forms (tri_geometry, below).
struct TriSide {
    int n;
    const uint8_t* desc;
    const orb_keypoint* kps;
    const uint8_t* has_mp;
    const float* uright;
    orb_featvec fv;
};
void tri_stage_pair(const TriSide& a, const TriSide& b, int only_stereo, TriItem* items, TriTrain* trains,
                    std::vector<int>& item_q, std::vector<int>& train_of) {
    for_common_nodes(a.fv, b.fv, [&](int na, int nb) {
        const int cb = (int)train_of.size();
        for (int i = b.fv.offsets[nb]; i < b.fv.offsets[nb + 1]; i++) {
            const int idx2 = b.fv.indices[i];
            if (b.has_mp[idx2]) continue;
            if (only_stereo && !(b.uright[idx2] >= 0)) continue;
            TriTrain& t = trains[train_of.size()];
            std::memcpy(t.desc, b.desc + (size_t)idx2 * 32, 32);
            t.x = b.kps[idx2].x;
            t.y = b.kps[idx2].y;
            t.sigma2 = (float)b.kps[idx2].octave;   // (the octave until tri_geometry)
            t.flags = b.uright[idx2] >= 0 ? 1 : 0;
            train_of.push_back(idx2);
        }
        const int ce = (int)train_of.size();
        if (ce == cb) return;
        for (int i = a.fv.offsets[na]; i < a.fv.offsets[na + 1]; i++) {
            const int idx1 = a.fv.indices[i];
            if (a.has_mp[idx1]) continue;                              // :694-696
            if (only_stereo && !(a.uright[idx1] >= 0)) continue;       // :698-702
            TriItem& q = items[item_q.size()];
            std::memcpy(q.desc, a.desc + (size_t)idx1 * 32, 32);
            q.la = a.kps[idx1].x;   // (the keypoint until tri_geometry)
            q.lb = a.kps[idx1].y;
            q.c0 = cb;
            q.c1 = ce;
            q.stereo = a.uright[idx1] >= 0 ? 1 : 0;
            item_q.push_back(idx1);
        }
    });
}

// The pair's float work on its staged records: each item's epipolar line (:143-145, contracted as
// tools/ref_flags_probe.cpp pins: a = fma(x, F00, y F10) + F20, b likewise, c = fma(y, F12, x F02) + F22), each
// train's epipole test (:743-748, fma(dex, dex, dey dey) < 100 scale) and sigma^2 (:156).  Every fma is exact
// whether it is an instruction or libm's fmaf, so the host picks the instruction when the CPU has it (a libm call
// costs ~3.5 ns: ~4 us per C3 call).
__attribute__((always_inline)) inline void tri_geometry_body(TriItem* items, int ib, int ie, TriTrain* trains, int tb,
                                                              int te, const float* F, float ex, float ey,
                                                              const float* scale2, const float* sigma2) {
    for (int i = ib; i < ie; i++) {
        TriItem& q = items[i];
        const float x = q.la, y = q.lb;
        tri_line(x, y, F, q.la, q.lb, q.lc);
    }
    for (int j = tb; j < te; j++) {
        TriTrain& t = trains[j];
        const int oct = (int)t.sigma2;
        if (tri_near_epipole(ex, ey, t.x, t.y, scale2, oct)) t.flags |= 2;
        t.sigma2 = tri_sigma2(sigma2, oct);
    }
}
#if !defined(__HIP_DEVICE_COMPILE__)   // (host code: the x86-64 FMA form and its dispatch)
__attribute__((target("fma"))) void tri_geometry_fma(TriItem* items, int ib, int ie, TriTrain* trains, int tb, int te,
                                                     const float* F, float ex, float ey, const float* scale2,
                                                     const float* sigma2) {
    tri_geometry_body(items, ib, ie, trains, tb, te, F, ex, ey, scale2, sigma2);
}
#endif
void tri_geometry(TriItem* items, int ib, int ie, TriTrain* trains, int tb, int te, const float* F, float ex, float ey,
                  const float* scale2, const float* sigma2) {
#if !defined(__HIP_DEVICE_COMPILE__)
    static const bool hw_fma = __builtin_cpu_supports("fma");
    if (hw_fma) return tri_geometry_fma(items, ib, ie, trains, tb, te, F, ex, ey, scale2, sigma2);
#endif
    tri_geometry_body(items, ib, ie, trains, tb, te, F, ex, ey, scale2, sigma2);
}

// One pair's acceptance from the kernel's per-item best records [ib, ie): rotation check (:792-813) and the pair list
// in ascending idx1 (:815-820).  Returns ORB_OK or ORB_ERR_CAPACITY (*npairs holds the full count either way).
int tri_replay_pair(Ctx* c, int check_ori, int n1, const orb_keypoint* kps1, const orb_keypoint* kps2, int ib, int ie,
                    const int* best, int* pairs_out, int cap, int* npairs) {
    const std::vector<int>& item_q = c->tri_item_q;
    std::vector<int>& vMatches12 = c->tri_match;
    vMatches12.assign(n1, -1);
    static_assert(HISTO_LENGTH == 30, "Ctx::tri_hist");
    std::vector<int>* rotHist = c->tri_hist;
    for (int i = 0; i < HISTO_LENGTH; i++) rotHist[i].clear();
    int nmatches = 0;
    for (int i = ib; i < ie; i++) {
        if (best[i] < 0) continue;
        const int idx1 = item_q[i];
        vMatches12[idx1] = best[i];
        nmatches++;
        if (check_ori) rotHist[rot_bin(kps1[idx1].angle, kps2[best[i]].angle)].push_back(idx1);
    }
    // :792-813 (no ">= 0" guard in this function: every culled entry decrements)
    if (check_ori) cull_rotation_all(rotHist, vMatches12, nmatches, -1);
    (void)nmatches;   // == the number of pairs collected below (:815-820)
    int np = 0;
    for (int i = 0; i < n1; i++) {
        if (vMatches12[i] < 0) continue;
        if (np < cap && pairs_out) {
            pairs_out[2 * np] = i;
            pairs_out[2 * np + 1] = vMatches12[i];
        }
        np++;
    }
    *npairs = np;
    return np > cap ? ORB_ERR_CAPACITY : ORB_OK;
}

// The pairs' staging (items and trains of every pair in one pinned mirror), one k_triangulation launch over all of
// them, one synchronisation, then each pair's replay.  A single call is the batch of one.
int tri_run(Ctx* c, int check_ori, int only_stereo, const TriSide& a, int npairs, const orb_tri_pair* pairs) {
    const int nnz1 = a.fv.nnodes > 0 ? a.fv.offsets[a.fv.nnodes] : 0;
    size_t cap_items = 0, cap_trains = 0;
    for (int p = 0; p < npairs; p++) {
        cap_items += (size_t)nnz1;
        cap_trains += pairs[p].fv2.nnodes > 0 ? (size_t)pairs[p].fv2.offsets[pairs[p].fv2.nnodes] : 0;
    }
    if (cap_items > (size_t)INT_MAX / 2 || cap_trains > (size_t)INT_MAX / 2)
        return arg_error("orb_search_for_triangulation", "too many records");
    std::vector<int>& item_q = c->tri_item_q;     // item -> idx1
    std::vector<int>& train_of = c->tri_train_of; // train record -> idx2
    item_q.clear();
    train_of.clear();
    std::vector<int>& ranges = c->tri_ranges;     // pair p's items: [ranges[p], ranges[p + 1])
    ranges.assign(npairs + 1, 0);
    Stage st{c};
    // the kernel reads the pinned mirror (zero copy) at every size: a DMA first measured slower for the single call
    // and for ten pairs alike (profiles/r06/triangulation_batch.txt)
    st.zc = 1;
    const size_t o_it = st.add(cap_items * sizeof(TriItem)), o_tr = st.add(cap_trains * sizeof(TriTrain)),
                 o_b = st.add(cap_items * 4);
    if (cap_items > 0 && cap_trains > 0) {
        const int r = st.alloc();
        if (r != ORB_OK) return r;
        TriItem* items = st.hi<TriItem>(o_it);
        TriTrain* trains = st.hi<TriTrain>(o_tr);
        for (int p = 0; p < npairs; p++) {
            const orb_tri_pair& P = pairs[p];
            const TriSide b{P.n2, P.desc2, P.kps2, P.has_mp2, P.uright2, P.fv2};
            const int tb = (int)train_of.size();
            tri_stage_pair(a, b, only_stereo, items, trains, item_q, train_of);
            ranges[p + 1] = (int)item_q.size();
            tri_geometry(items, ranges[p], ranges[p + 1], trains, tb, (int)train_of.size(), P.F12, P.ex, P.ey, P.scale2,
                         P.sigma2_2);
        }
    }
    const int nitems = (int)item_q.size();
    std::vector<int>& best = c->tri_best;
    best.assign(nitems, -1);
    if (nitems) {
        if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 1, c->stream);
        hipError_t e = launch_triangulation(st.di<TriItem>(o_it), st.di<TriTrain>(o_tr), nitems, st.h<int>(o_b), c->stream);
        if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 0, c->stream);
        if (e != hipSuccess) return set_error("triangulation kernel", e), ORB_ERR_HIP;
        // the kernel writes its results straight into the pinned mirror (host-coherent memory): no D2H command
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess)
            return set_error("download", e), ORB_ERR_HIP;
        const int* hb = st.h<int>(o_b);
        for (int i = 0; i < nitems; i++) best[i] = hb[i] >= 0 ? train_of[hb[i]] : -1;
    }
    int rc = ORB_OK;
    for (int p = 0; p < npairs; p++) {
        const orb_tri_pair& P = pairs[p];
        if (tri_replay_pair(c, check_ori, a.n, a.kps, P.kps2, ranges[p], ranges[p + 1], best.data(), P.pairs_out,
                            P.cap, P.npairs) != ORB_OK)
            rc = ORB_ERR_CAPACITY;
    }
    if (rc != ORB_OK) set_error("pairs_out too small", hipSuccess);
    return rc;
}

// A pair of the host-pointer forms.  tri_geometry_body indexes scale2 / sigma2_2 with the octave of the KF2 keypoints
// the staging reads: every KF2 keypoint's octave lies in [0, nlevels2), as the _frames form asks of a frame (one
// sequential pass without a branch: about half the time of a pass over fv2.indices).
bool tri_pair_ok(const orb_tri_pair& P) {
    if (!(P.n2 >= 0 && P.npairs && P.nlevels2 >= 1 && P.nlevels2 <= ORBGPU_MAX_LEVELS && P.F12 && P.scale2 &&
          P.sigma2_2 && featvec_ok(P.fv2, P.n2) && (P.n2 == 0 || (P.desc2 && P.kps2 && P.has_mp2 && P.uright2))))
        return false;
    int bad = 0;
    for (int i = 0; i < P.n2; i++) bad += (unsigned)P.kps2[i].octave >= (unsigned)P.nlevels2;
    return bad == 0;
}
}  // namespace
}  // namespace orbgpu

extern "C" {

int orb_search_for_triangulation(orb_ctx* h, int check_ori, int only_stereo, int n1, const uint8_t* desc1,
                                 const orb_keypoint* kps1, const uint8_t* has_mp1, const float* uright1,
                                 orb_featvec fv1, int n2, const uint8_t* desc2, const orb_keypoint* kps2,
                                 const uint8_t* has_mp2, const float* uright2, orb_featvec fv2, const float* F12,
                                 float ex, float ey, const float* scale2, const float* sigma2_2, int nlevels2,
                                 int* pairs_out, int cap, int* npairs) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (n1 < 0) return ORB_ERR_ARG;
    if (!featvec_ok(fv1, n1)) return arg_error("orb_search_for_triangulation", "malformed FeatureVector CSR");
    const orb_tri_pair P{n2, desc2, kps2, has_mp2, uright2, fv2, F12, ex, ey, scale2, sigma2_2, nlevels2, pairs_out, cap,
                         npairs};
    if (!tri_pair_ok(P))
        return arg_error("orb_search_for_triangulation", "bad pair arguments (or a KF2 octave outside [0, nlevels2))");
    return tri_run(c, check_ori, only_stereo, TriSide{n1, desc1, kps1, has_mp1, uright1, fv1}, 1, &P);
}

int orb_search_for_triangulation_batch(orb_ctx* h, int check_ori, int only_stereo, int n1, const uint8_t* desc1,
                                       const orb_keypoint* kps1, const uint8_t* has_mp1, const float* uright1,
                                       orb_featvec fv1, int npairs, const orb_tri_pair* pairs) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (n1 < 0 || npairs < 0 || (npairs > 0 && !pairs)) return ORB_ERR_ARG;
    if (!featvec_ok(fv1, n1)) return arg_error("orb_search_for_triangulation_batch", "malformed FeatureVector CSR");
    for (int p = 0; p < npairs; p++)
        if (!tri_pair_ok(pairs[p]))
            return arg_error("orb_search_for_triangulation_batch",
                             "bad pair arguments (or a KF2 octave outside [0, nlevels2))");
    if (npairs == 0) return ORB_OK;
    return tri_run(c, check_ori, only_stereo, TriSide{n1, desc1, kps1, has_mp1, uright1, fv1}, npairs, pairs);
}

int orb_search_for_triangulation_frames(orb_ctx* h, int check_ori, int only_stereo, const orb_frame* F1,
                                        const uint8_t* has_mp1, int npairs, const orb_tri_frame_pair* pairs) {
    const char* const fn = "orb_search_for_triangulation_frames";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    const auto side_fault = [](const orb_frame* F) -> const char* {
        if (!F) return "NULL frame";
        if (!F->bow) return "a frame carries no BoW";
        if (!F->has_ur) return "a frame was created without uright";
        return nullptr;
    };
    if (npairs < 0 || npairs > 65535 || (npairs > 0 && !pairs)) return arg_error(fn, "bad arguments");
    for (int p = 0; p < npairs; p++)
        if (pairs[p].nlevels2 < 1 || pairs[p].nlevels2 > ORBGPU_MAX_LEVELS)
            return arg_error(fn, "nlevels2 outside [1, ORBGPU_MAX_LEVELS]");
    if (const char* why = side_fault(F1)) return arg_error(fn, why);
    // k_triangulation_frames finds a KF1 feature's node in a per-feature array: one node per feature
    if (!F1->bow->unique) return arg_error(fn, "frame1's FeatureVector lists a feature twice");
    if (F1->n > 0 && !has_mp1) return arg_error(fn, "bad arguments");
    for (int p = 0; p < npairs; p++) {
        const orb_tri_frame_pair& P = pairs[p];
        if (const char* why = side_fault(P.frame2)) return arg_error(fn, why);
        if (P.frame2->device != F1->device) return arg_error(fn, "frames of different devices");
        if (!P.npairs || !P.F12 || !P.scale2 || !P.sigma2_2 || (P.frame2->n > 0 && !P.has_mp2))
            return arg_error(fn, "bad pair arguments");
        // the kernel indexes scale2 / sigma2_2 with the octaves of frame2's keypoints
        if (P.frame2->n > 0 && (P.frame2->oct_min < 0 || P.frame2->oct_max >= P.nlevels2))
            return arg_error(fn, "a frame2 octave outside [0, nlevels2)");
    }
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    if (F1->device != c->device) return arg_error(fn, "frame of another device");
    CTX_GUARD(c);
    if (npairs == 0) return ORB_OK;
    const int n1 = F1->n;
    const orb_frame_bow* B1 = F1->bow;
    // [table | has_mp1 | has_mp2 ...] go up in one DMA (every candidate's flag is read by each KF1 feature of its
    // node: device memory, not the pinned mirror); the kernel stores its results into the mirror
    Stage st{c};
    const size_t o_tab = st.add((size_t)npairs * sizeof(TriFramePair)), o_f1 = st.add((size_t)n1);
    std::vector<size_t> o_f2(npairs);
    for (int p = 0; p < npairs; p++) o_f2[p] = st.add((size_t)pairs[p].frame2->n);
    const size_t in_end = st.off, o_out = st.add((size_t)npairs * (size_t)n1 * 4);
    if (n1 > 0) {
        if ((size_t)npairs * (size_t)n1 > (size_t)INT_MAX / 2) return arg_error(fn, "too many records");
        const int r = st.alloc();
        if (r != ORB_OK) return r;
        TriFramePair* tab = st.hi<TriFramePair>(o_tab);
        st.put(o_f1, has_mp1, (size_t)n1);
        for (int p = 0; p < npairs; p++) {
            const orb_tri_frame_pair& P = pairs[p];
            const orb_frame* F2 = P.frame2;
            const orb_frame_bow* B2 = F2->bow;
            st.put(o_f2[p], P.has_mp2, (size_t)F2->n);
            TriFramePair& T = tab[p];
            T = TriFramePair{};
            T.desc = F2->d_desc;
            T.kps = F2->d_kps;
            T.ur = F2->d_ur;
            T.fv_nodes = B2->d<uint32_t>(B2->L.o_nodes);
            T.fv_off = B2->d<int>(B2->L.o_off);
            T.fv_idx = B2->d<int>(B2->L.o_idx);
            T.has_mp = st.d<uint8_t>(o_f2[p]);
            T.nnodes = B2->nnodes;
            T.ex = P.ex;
            T.ey = P.ey;
            std::memcpy(T.F, P.F12, sizeof(T.F));
            std::memcpy(T.scale2, P.scale2, (size_t)P.nlevels2 * 4);
            std::memcpy(T.sigma2, P.sigma2_2, (size_t)P.nlevels2 * 4);
        }
        hipError_t e;
        if ((e = st.up(0, in_end)) != hipSuccess) return set_error("upload", e), ORB_ERR_HIP;
        const TriFrameKf1 A{F1->d_desc, F1->d_kps, F1->d_ur, B1->d<uint32_t>(B1->L.o_nodeof), st.d<uint8_t>(o_f1), n1};
        if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 1, c->stream);
        e = launch_triangulation_frames(A, st.d<TriFramePair>(o_tab), npairs, only_stereo, st.h<int>(o_out), c->stream);
        if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 0, c->stream);
        if (e != hipSuccess) return set_error("triangulation kernel", e), ORB_ERR_HIP;
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return set_error("download", e), ORB_ERR_HIP;
    }
    // the replay's items: KF1's FeatureVector in CSR order, once per pair (a feature outside it matches nothing)
    const orb_featvec fv1 = B1->featvec();
    const int nnz1 = B1->nnz;
    std::vector<int>& item_q = c->tri_item_q;
    std::vector<int>& best = c->tri_best;
    item_q.resize((size_t)npairs * nnz1);
    best.resize((size_t)npairs * nnz1);
    const int* out = n1 > 0 ? st.h<int>(o_out) : nullptr;
    int rc = ORB_OK;
    for (int p = 0; p < npairs; p++) {
        const orb_tri_frame_pair& P = pairs[p];
        const size_t ib = (size_t)p * nnz1;
        for (int k = 0; k < nnz1; k++) {
            item_q[ib + k] = fv1.indices[k];
            best[ib + k] = out[(size_t)p * n1 + fv1.indices[k]];
        }
        if (tri_replay_pair(c, check_ori, n1, F1->kps.data(), P.frame2->kps.data(), (int)ib, (int)ib + nnz1, best.data(),
                            P.pairs_out, P.cap, P.npairs) != ORB_OK)
            rc = ORB_ERR_CAPACITY;
    }
    if (rc != ORB_OK) set_error("pairs_out too small", hipSuccess);
    return rc;
}

}  // extern "C"

namespace orbgpu {
namespace {
// The window searches' acceptance, replayed in the reference's query order (:440-498): first / second
// admissible candidate, vMatchedDistance stealing, rotation histogram.
int window_replay(TopkSession& s, float nnratio, int check_ori, int n1, const orb_keypoint* kps1, int n2,
                  const orb_keypoint* kps2, int* match12, int* nmatches_out) {
    int st = s.run(0, nullptr);
    if (st != ORB_OK) return st;
    std::vector<int> vnMatches12(n1, -1), vnMatches21(n2, -1), vMatchedDistance(n2, INT_MAX);
    std::vector<int> rotHist[HISTO_LENGTH];
    int nmatches = 0;
    auto admit = [&](int t, int d) { return vMatchedDistance[t] > d; };   // if(vMatchedDistance[i2]<=dist) continue;
    auto fill_thr = [&]() { return vMatchedDistance.data(); };   // the kernel's own rule is thr[t] <= d: skip
    TopkPick p;
    for (int i = 0; i < s.nitems; i++) {
        if ((st = s.pick(i, 2, admit, kTopkNoStop, fill_thr, -1, p)) != ORB_OK) return st;
        const int d1 = p.dist(0, INT_MAX), b2 = p.t[0], d2 = p.dist(1, INT_MAX);   // bestDist = bestDist2 = INT_MAX
        const int i1 = s.item_q[i];
        if (d1 <= TH_LOW && d1 < (float)d2 * nnratio) {   // :457-459
            if (vnMatches21[b2] >= 0) {
                vnMatches12[vnMatches21[b2]] = -1;
                nmatches--;
            }
            vnMatches12[i1] = b2;
            vnMatches21[b2] = i1;
            vMatchedDistance[b2] = d1;
            nmatches++;
            if (check_ori) rotHist[rot_bin(kps1[i1].angle, kps2[b2].angle)].push_back(i1);
        }
    }
    if (check_ori) cull_rotation(rotHist, vnMatches12, nmatches);
    std::memcpy(match12, vnMatches12.data(), (size_t)n1 * sizeof(int));
    if (nmatches_out) *nmatches_out = nmatches;
    return ORB_OK;
}

// The projection-gated searches' acceptance from the top-k lists, in query order.  A train is taken (skipped, as
// `if(mvpMapPoints[i]) if(Observations()>0) continue;` does, :87-89 / :1403-1405 / :1963-1965) if the caller marked
// it or an earlier query with blocks != 0 was assigned to it; an assignment by a query with blocks == 0 leaves it
// open, and a later one overwrites it (both count).  A list the taken set exhausts while the window holds more
// than K admissible candidates is re-ranked on the GPU from that query on, as bow_kf_f_replay does.
int proj_replay(TopkSession& s, int mode, float nnratio, int check_ori, int max_dist, const orb_proj_query* q,
                const orb_keypoint* kps_t, const uint8_t* t_taken, int* match_t, int* nmatches_out) {
    const int nq = s.nitems, nt = s.nt;
    std::vector<char> taken(nt, 0);
    std::vector<int> thr(nt), matches(nt, -1);
    std::vector<int> rotHist[HISTO_LENGTH];
    auto fill_thr = [&]() {
        for (int t = 0; t < nt; t++) thr[t] = taken[t] ? -1 : INT_MAX;
        return thr.data();
    };
    if (t_taken)
        for (int t = 0; t < nt; t++) taken[t] = t_taken[t] != 0;
    int st = s.run(0, t_taken ? fill_thr() : nullptr);
    if (st != ORB_OK) return st;
    // SearchByProjection(CurrentFrame, LastFrame) keeps one minimum, the other forms two; all of them start at 256
    // and update on '<' only, so an entry at 256 or beyond ends the entries that can be a minimum
    const int need = mode == ORB_PROJ_BEST ? 1 : 2;
    auto admit = [&](int t, int) { return !taken[t]; };
    TopkPick p;
    int nmatches = 0;
    for (int i = 0; i < nq; i++) {
        if ((st = s.pick(i, need, admit, 256, fill_thr, -1, p)) != ORB_OK) return st;
        const int found = p.found;
        const int* d = p.d;
        const int* ti = p.t;
        if (found == 0 || d[0] > max_dist) continue;   // :118 / :1426 / :1987
        if (mode == ORB_PROJ_RATIO_SAME_LEVEL) {       // :120-121 / :1989-1990
            const int bestLevel = kps_t[ti[0]].octave, bestLevel2 = found == 2 ? kps_t[ti[1]].octave : -1;
            const int bestDist2 = found == 2 ? d[1] : 256;
            if (bestLevel == bestLevel2 && static_cast<float>(d[0]) > nnratio * static_cast<float>(bestDist2)) continue;
        }
        matches[ti[0]] = i;
        taken[ti[0]] = q[i].blocks != 0;
        nmatches++;
        if (mode == ORB_PROJ_BEST && check_ori) rotHist[rot_bin(q[i].angle, kps_t[ti[0]].angle)].push_back(ti[0]);
    }
    // :1448-1467: every entry of a culled bin resets its train and decrements (no guard: a train entered twice by
    // overwriting queries counts twice)
    if (mode == ORB_PROJ_BEST && check_ori) cull_rotation_all(rotHist, matches, nmatches, -2);
    std::memcpy(match_t, matches.data(), (size_t)nt * sizeof(int));
    if (nmatches_out) *nmatches_out = nmatches;
    return ORB_OK;
}

// SearchByMatchBird(KeyFrame*, Frame&, ...)'s acceptance (ORBmatcher.cc:2014-2111) from the top-k lists, in query
// order.  Unlike proj_replay there is no taken set and no cut at 256: a candidate is skipped when
// vMatchedDistanceBird[idx] <= dist (:2051), the running minima start at INT_MAX, a closer later query overwrites a
// train without giving the count back, and the rotation histogram holds trains, the same one twice after a steal.
// The (dist, slot) order of a list is the order of the reference's strict-'<' updates, so its first two admissible
// entries are (bestDist, bestIdx, bestLevel) and (bestDist2, bestLevel2).  A list that cannot give both while the
// window held more than K candidates is re-ranked on the GPU from that query on against the current table, as
// window_replay does (the table only decreases, so an entry the kernel dropped stays inadmissible).
int match_bird_replay(TopkSession& s, float nnratio, int check_ori, int max_dist, const int* q_id,
                      const float* q_angle, const orb_keypoint* kps_t, int* match_t, int* nmatches_out) {
    const int nq = s.nitems, nt = s.nt;
    int st = s.run(0, nullptr);
    if (st != ORB_OK) return st;
    std::vector<int> vMatchedDistanceBird(nt, INT_MAX), matches(nt, -1);
    std::vector<int> rotHist[HISTO_LENGTH];
    auto admit = [&](int t, int d) { return vMatchedDistanceBird[t] > d; };   // :2051
    auto fill_thr = [&]() { return vMatchedDistanceBird.data(); };
    TopkPick p;
    int nmatches = 0;
    for (int i = 0; i < nq; i++) {
        if ((st = s.pick(i, 2, admit, kTopkNoStop, fill_thr, -1, p)) != ORB_OK) return st;
        if (p.found == 0) continue;   // :2025, or every candidate skipped: bestDist stays INT_MAX
        const int bestDist = p.d[0], bestIdx = p.t[0], bestLevel = kps_t[bestIdx].octave;
        const int bestDist2 = p.dist(1, INT_MAX), bestLevel2 = p.found == 2 ? kps_t[p.t[1]].octave : -1;
        if (bestDist <= max_dist) {                                                      // :2070
            if (bestLevel != bestLevel2 || bestDist < (float)bestDist2 * nnratio) {      // :2072
                matches[bestIdx] = q_id ? q_id[i] : i;
                vMatchedDistanceBird[bestIdx] = bestDist;
                if (check_ori) rotHist[rot_bin(q_angle[i], kps_t[bestIdx].angle)].push_back(bestIdx);
                nmatches++;
            }
        }
    }
    if (check_ori) cull_rotation_all(rotHist, matches, nmatches, -2);   // :2093-2111, no guard
    std::memcpy(match_t, matches.data(), (size_t)nt * sizeof(int));
    if (nmatches_out) *nmatches_out = nmatches;
    return ORB_OK;
}

// The per-query validators of the grid searches (nothing malformed may reach the device): each returns what is wrong,
// or NULL.  Queries [q0, q1) of the projection searches: a finite window with a radius >= 0, and with gate FUSE a
// finite ur.
const char* proj_queries_fault(const orb_proj_query* q, int q0, int q1, bool fuse = false) {
    for (int i = q0; i < q1; i++) {
        if (!std::isfinite(q[i].u) || !std::isfinite(q[i].v) || !std::isfinite(q[i].r) || q[i].r < 0)
            return "query window not finite or radius negative";
        if (fuse && !std::isfinite(q[i].ur)) return "query ur not finite";
    }
    return nullptr;
}
// SearchByMatchBird's queries: finite centres, and ids >= 0 (match_t keeps the negative values for "untouched" and
// "culled").
const char* bird_queries_fault(int nq, const float* q_xy, const int* q_id) {
    for (int i = 0; i < nq; i++) {
        if (!std::isfinite(q_xy[2 * i]) || !std::isfinite(q_xy[2 * i + 1])) return "query centre not finite";
        if (q_id && q_id[i] < 0) return "negative query id";
    }
    return nullptr;
}
// The scalars the projection searches and SearchByMatchBird check first, ahead of a NULL frame.
const char* max_dist_fault(int max_dist) {
    return max_dist < 0 || max_dist > 256 ? "max_dist outside [0, 256]" : nullptr;
}
const char* proj_scalars_fault(int mode, int max_dist) {
    if (mode != ORB_PROJ_BEST && mode != ORB_PROJ_RATIO_SAME_LEVEL) return "unknown mode";
    return max_dist_fault(max_dist);
}
const char* bird_scalars_fault(int max_dist, float r) {
    if (const char* why = max_dist_fault(max_dist)) return why;
    return !std::isfinite(r) || r < 0 ? "radius not finite or negative" : nullptr;
}

// k_projection_topk's lanes per query: a wavefront per query measured 3-4 us per call faster than a query per 16-lane
// row at 640x480 / 1,000 queries and level with it at 1280x720 / 2,000, so it is the form in use;
// ORBGPU_PROJ_LANES=16 selects the row form (diagnostic: profiles/time_projection.py times both)
int proj_lanes() {
    const char* e = getenv("ORBGPU_PROJ_LANES");
    return (e && atoi(e) == 16) ? 16 : 64;
}

// The context of a grid search (after the argument checks, before anything is written): not NULL, the device a
// resident train side lives on, and that device made current.
int side_guard(const char* fn, const Ctx* c, const TrainSide& side) {
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    if (side.on_other_device(c)) return arg_error(fn, "the frame lives on another device");
    CTX_GUARD(c);
    return ORB_OK;
}

// A target of the per-query searches as both entry points give it: its queries and outputs, and its train side.
struct ProjView {
    int nq;
    const orb_proj_query* q;
    const uint8_t* qdesc;
    const float* inv_sigma2;
    int nlevels;
    int* best_idx;
    int* best_dist;
    TrainSide side;
};
ProjView proj_view(const orb_proj_target& T) {
    return ProjView{T.nq, T.q, T.qdesc, T.inv_sigma2, T.nlevels, T.best_idx, T.best_dist,
                    TrainSide(T.nt, T.tdesc, T.kps_t, T.t_uright, T.grid)};
}
ProjView proj_view(const orb_proj_frame_target& R) {   // (R.frame != NULL; its uright gates as a host target's does)
    return ProjView{R.nq, R.q, R.qdesc, R.inv_sigma2, R.nlevels, R.best_idx, R.best_dist, TrainSide(R.frame, true)};
}

// What is wrong with a target of orb_project_best_batch / orb_project_best_frames for its queries [q0, q1), or NULL.
// The kernel indexes inv_sigma2 by the train's octave and the trains by the grid's cell_idx, so both are checked here.
const char* proj_target_fault(int gate, const ProjView& V, int q0, int q1) {
    const TrainSide& S = V.side;
    if (V.nq < 0 || S.n < 0) return "negative count";
    if (V.nq > 0 && (!V.best_idx || !V.best_dist)) return "NULL outputs";
    if (V.nq > 0 && (!V.q || !V.qdesc)) return "bad arguments";
    if (const char* why = S.fault()) return why;
    if (const char* why = proj_queries_fault(V.q, q0, q1, gate == ORB_PROJ_GATE_FUSE)) return why;
    if (gate == ORB_PROJ_GATE_FUSE) {
        if (!V.inv_sigma2) return "inv_sigma2 NULL";
        if (V.nlevels < 1 || V.nlevels > ORBGPU_MAX_LEVELS) return "nlevels outside [1, ORBGPU_MAX_LEVELS]";
        for (int t = 0; t < S.n; t++)
            if (S.kps[t].octave < 0 || S.kps[t].octave >= V.nlevels) return "train octave outside [0, nlevels)";
    }
    return nullptr;
}

// One query of a (validated) target on the CPU: k_projection_best's walk over the grid CSR (grid_window.h),
// sequentially.
void proj_best_one(int gate, const orb_proj_target& T, const orb_proj_query& P, const uint8_t* qdesc, int* best_idx,
                   int* best_dist) {
    const orb_frame_grid& g = T.grid;
    *best_idx = -1;
    *best_dist = -1;
    const float x = P.u, y = P.v, r = P.r;
    const CellRect c = cell_rect(x, y, r, g.min_x, g.min_y, g.inv_w, g.inv_h);
    if (c.empty) return;
    int bestDist = INT_MAX, bestIdx = -1;
    for (int ix = c.x0; ix <= c.x1; ix++)
        for (int s = g.cell_off[ix * kFrameGridRows + c.y0]; s < g.cell_off[ix * kFrameGridRows + c.y1 + 1]; s++) {
            const int ti = g.cell_idx[s];
            const orb_keypoint& kp = T.kps_t[ti];
            if (!window_admits(kp, x, y, r, P.min_level, P.max_level)) continue;
            if (gate == ORB_PROJ_GATE_FUSE && fuse_gate_skips(x, y, P.ur, kp.x, kp.y, T.t_uright ? T.t_uright[ti] : -1.0f,
                                                              T.inv_sigma2[kp.octave]))
                continue;
            const int d = orb_descriptor_distance(qdesc, T.tdesc + (size_t)ti * 32);
            if (d < bestDist) {
                bestDist = d;
                bestIdx = ti;
            }
        }
    if (bestIdx >= 0) {
        *best_idx = bestIdx;
        *best_dist = bestDist;
    }
}

// The bodies of the grid searches, one per search for both forms of the train side.  An entry point checks what only
// its form has (the host arrays and their grid, or the frame) and calls its body under its own name fn; the arguments
// are checked before the context, so nothing malformed reaches the device and no output is written: k_window_topk and
// k_projection_topk read cell_idx[cell_off[..]] for every rectangle column.

// orb_window_match_grid / orb_window_match_frame (and orb_search_by_match_bird_frame's matching)
int window_grid_run(const char* fn, orb_ctx* h, float nnratio, int check_ori, int level0_only, int n1,
                    const uint8_t* desc1, const orb_keypoint* kps1, const float* centres, float window,
                    const TrainSide& side, int* match12, int* nmatches_out) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const int st = side_guard(fn, c, side)) return st;
    if (n1 == 0 || side.n == 0) {
        for (int i = 0; i < n1; i++) match12[i] = -1;
        if (nmatches_out) *nmatches_out = 0;
        return ORB_OK;
    }
    TopkSession s{c};
    for (int i1 = 0; i1 < n1; i1++) {
        if (level0_only && kps1[i1].octave > 0) continue;   // :420-423 (a query without candidates ranks nothing)
        s.item_q.push_back(i1);
    }
    const int st = s.setup_grid(desc1, n1, kps1, centres, window, side);
    if (st != ORB_OK) return st;
    return window_replay(s, nnratio, check_ori, n1, kps1, side.n, side.kps, match12, nmatches_out);
}

// orb_search_by_projection / orb_search_by_projection_frame, after mode and max_dist
int projection_search_run(const char* fn, orb_ctx* h, int mode, float nnratio, int check_ori, int max_dist, int nq,
                          const orb_proj_query* q, const uint8_t* qdesc, const TrainSide& side, const uint8_t* t_taken,
                          int* match_t, int* nmatches_out) {
    if (const char* why = proj_queries_fault(q, 0, nq)) return arg_error(fn, why);
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const int st = side_guard(fn, c, side)) return st;
    for (int t = 0; t < side.n; t++) match_t[t] = -1;
    if (nmatches_out) *nmatches_out = 0;
    if (nq == 0 || side.n == 0) return ORB_OK;
    TopkSession s{c};
    const int st = s.setup_proj(nq, q, qdesc, side, proj_lanes());
    if (st != ORB_OK) return st;
    return proj_replay(s, mode, nnratio, check_ori, max_dist, q, side.kps, t_taken, match_t, nmatches_out);
}

// orb_search_by_match_bird / orb_search_by_match_bird_resident, after max_dist and r: k_projection_topk over the
// birdview grid (a wavefront per query, no stereo gate), the acceptance is match_bird_replay
int match_bird_run(const char* fn, orb_ctx* h, float nnratio, int check_ori, int max_dist, float r, int nq,
                   const int* q_id, const float* q_xy, const float* q_angle, const uint8_t* qdesc, const TrainSide& side,
                   int* match_t, int* nmatches_out) {
    if (const char* why = bird_queries_fault(nq, q_xy, q_id)) return arg_error(fn, why);
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (const int st = side_guard(fn, c, side)) return st;
    for (int t = 0; t < side.n; t++) match_t[t] = -1;
    if (nmatches_out) *nmatches_out = 0;
    if (nq == 0 || side.n == 0) return ORB_OK;
    std::vector<orb_proj_query> q(nq);
    for (int i = 0; i < nq; i++)   // GetFeaturesInAreaBirdview(pt.x, pt.y, r): the default levels (:2023)
        q[i] = orb_proj_query{q_xy[2 * i], q_xy[2 * i + 1], r, -1, -1, 0.0f, 0.0f, 0.0f, 0};
    TopkSession s{c};
    const int st = s.setup_proj(nq, q.data(), qdesc, side, 64);
    if (st != ORB_OK) return st;
    return match_bird_replay(s, nnratio, check_ori, max_dist, q_id, q_angle, side.kps, match_t, nmatches_out);
}
}  // namespace
}  // namespace orbgpu

extern "C" {

/* SearchForInitialization (:405-520) / BirdviewMatch(const Frame&, const Frame&, ...) (:1790-1899) */
int orb_window_match(orb_ctx* h, float nnratio, int check_ori, int level0_only, int n1, const uint8_t* desc1,
                     const orb_keypoint* kps1, int n2, const uint8_t* desc2, const orb_keypoint* kps2,
                     const int* cand_off, const int* cand_idx, int* match12, int* nmatches_out) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    if (n1 < 0 || n2 < 0 || !match12 || !cand_off) return ORB_ERR_ARG;
    TopkSession s{c};
    s.cand = cand_idx;
    s.ncand = cand_off[n1];
    for (int i1 = 0; i1 < n1; i1++) {
        if (level0_only && kps1[i1].octave > 0) continue;   // :420-423
        if (cand_off[i1 + 1] == cand_off[i1]) continue;     // :427-428
        s.item_q.push_back(i1);
        s.item_rng.push_back(make_int2(cand_off[i1], cand_off[i1 + 1]));
    }
    const int st = s.setup(desc1, desc2, n2);
    if (st != ORB_OK) return st;
    return window_replay(s, nnratio, check_ori, n1, kps1, n2, kps2, match12, nmatches_out);
}

/* The same searches with GetFeaturesInArea computed on the device from F2's grid (orbgpu.h). */
int orb_window_match_grid(orb_ctx* h, float nnratio, int check_ori, int level0_only, int n1, const uint8_t* desc1,
                          const orb_keypoint* kps1, const float* centres, float window, int n2,
                          const uint8_t* desc2, const orb_keypoint* kps2, orb_frame_grid grid2, int* match12,
                          int* nmatches_out) {
    const char* const fn = "orb_window_match_grid";
    if (n1 < 0 || n2 < 0 || !match12 || (n1 && (!desc1 || !kps1))) return arg_error(fn, "bad arguments");
    const TrainSide side(n2, desc2, kps2, nullptr, grid2);
    if (const char* why = side.fault()) return arg_error(fn, why);
    return window_grid_run(fn, h, nnratio, check_ori, level0_only, n1, desc1, kps1, centres, window, side, match12,
                           nmatches_out);
}

/* SearchByProjection(Frame&, const Frame&, th, bMono) (:1328-1470), SearchByProjection(Frame&, vector<MapPoint*>, th)
 * (:45-129) and SearchByProjectionBird (:1923-1998) over one core (orbgpu.h has the mappings). */
int orb_search_by_projection(orb_ctx* h, int mode, float nnratio, int check_ori, int max_dist, int nq,
                             const orb_proj_query* q, const uint8_t* qdesc, int nt, const uint8_t* tdesc,
                             const orb_keypoint* kps_t, const float* t_uright, const uint8_t* t_taken,
                             orb_frame_grid grid, int* match_t, int* nmatches_out) {
    const char* const fn = "orb_search_by_projection";
    if (const char* why = proj_scalars_fault(mode, max_dist)) return arg_error(fn, why);
    if (nq < 0 || nt < 0 || (nt && !match_t) || (nq && (!q || !qdesc))) return arg_error(fn, "bad arguments");
    const TrainSide side(nt, tdesc, kps_t, t_uright, grid);
    if (const char* why = side.fault()) return arg_error(fn, why);
    return projection_search_run(fn, h, mode, nnratio, check_ori, max_dist, nq, q, qdesc, side, t_taken, match_t,
                                 nmatches_out);
}

/* SearchByMatchBird(KeyFrame*, Frame&, vector<MapPointBird*>&, r) (:2000-2114): the grid walk and the ranking are
 * orb_search_by_projection's (k_projection_topk over the birdview grid, levels (-1, -1), no stereo gate), the
 * acceptance is match_bird_replay. */
int orb_search_by_match_bird(orb_ctx* h, float nnratio, int check_ori, int max_dist, float r, int nq, const int* q_id,
                             const float* q_xy, const float* q_angle, const uint8_t* qdesc, int nt,
                             const uint8_t* tdesc, const orb_keypoint* kps_t, orb_frame_grid grid, int* match_t,
                             int* nmatches_out) {
    const char* const fn = "orb_search_by_match_bird";
    if (const char* why = bird_scalars_fault(max_dist, r)) return arg_error(fn, why);
    if (nq < 0 || nt < 0 || (nt && !match_t) || (nq && (!q_xy || !qdesc || (check_ori && !q_angle))))
        return arg_error(fn, "bad arguments");
    const TrainSide side(nt, tdesc, kps_t, nullptr, grid);
    if (const char* why = side.fault()) return arg_error(fn, why);
    return match_bird_run(fn, h, nnratio, check_ori, max_dist, r, nq, q_id, q_xy, q_angle, qdesc, side, match_t,
                          nmatches_out);
}

/* SearchByMatchBird(Frame& CurrentFrame, const Frame& LastFrame, windowSize) (:1901-1921): BirdviewMatch(LastFrame,
 * CurrentFrame, ...) through orb_window_match_grid's path, then the carry-over of mvpMapPointsBird on the host. */
int orb_search_by_match_bird_frame(orb_ctx* h, float nnratio, int check_ori, float window, int n_last,
                                   const uint8_t* desc_last, const orb_keypoint* kps_last, const uint8_t* has_mp_last,
                                   int n_cur, const uint8_t* desc_cur, const orb_keypoint* kps_cur,
                                   orb_frame_grid grid_cur, int* match_cur, int* nmatches_out) {
    const char* const fn = "orb_search_by_match_bird_frame";
    if (n_last < 0 || n_cur < 0 || (n_cur && !match_cur) || (n_last && (!desc_last || !kps_last)))
        return arg_error(fn, "bad arguments");
    const TrainSide side(n_cur, desc_cur, kps_cur, nullptr, grid_cur);
    if (const char* why = side.fault()) return arg_error(fn, why);
    Ctx* c = reinterpret_cast<Ctx*>(h);
    CTX_GUARD(c);
    std::vector<int> vnMatches12((size_t)std::max(n_last, 1), -1);
    if (has_mp_last && n_last > 0 && n_cur > 0) {   // (without map points nothing is carried whatever matches)
        const int st = window_grid_run(fn, h, nnratio, check_ori, 0, n_last, desc_last, kps_last, nullptr, window, side,
                                       vnMatches12.data(), nullptr);
        if (st != ORB_OK) return st;
    }
    int nmatches = 0;
    for (int t = 0; t < n_cur; t++) match_cur[t] = -1;
    for (int k = 0; k < n_last && has_mp_last; k++) {   // :1907-1918
        const int idx2 = vnMatches12[k];
        if (idx2 < 0) continue;
        if (has_mp_last[k]) {
            match_cur[idx2] = k;
            nmatches++;
        }
    }
    if (nmatches_out) *nmatches_out = nmatches;
    return ORB_OK;
}

}  // extern "C"

namespace orbgpu {
namespace {
// orb_project_best_batch and orb_project_best_frames over their common view of the targets (fn: the entry point's
// name for messages).
int project_best_run(const char* fn, orb_ctx* h, int gate, const std::vector<ProjView>& targets) {
    // everything is checked before the context and before any output is written: nothing runs if a target is malformed
    const int ntargets = (int)targets.size();
    size_t nitems = 0, nused = 0;
    for (int k = 0; k < ntargets; k++) {
        const ProjView& V = targets[k];
        if (const char* why = proj_target_fault(gate, V, 0, V.nq))
            return arg_error(fn, "target " + std::to_string(k) + ": " + why);
        if (V.nq > 0 && V.side.n > 0) {
            nitems += (size_t)V.nq;
            nused++;
        }
    }
    if (nitems > (size_t)INT_MAX / 2) return arg_error(fn, "too many queries");
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    for (int k = 0; k < ntargets; k++)
        if (targets[k].side.on_other_device(c))
            return arg_error(fn, "target " + std::to_string(k) + ": the frame lives on another device");
    CTX_GUARD(c);
    for (int k = 0; k < ntargets; k++)
        for (int i = 0; i < targets[k].nq; i++) targets[k].best_idx[i] = targets[k].best_dist[i] = -1;
    if (nitems == 0) return ORB_OK;
    // the staging area: [table | item -> table row | queries | query descriptors | per used target: descriptors,
    // keypoints, uright, inv_sigma2, cell_off, cell_idx (a resident frame: inv_sigma2 only)] in one DMA, then the
    // outputs the kernel writes into the mirror
    const bool fuse = gate == ORB_PROJ_GATE_FUSE;
    Stage st{c};
    const size_t o_tab = st.add(nused * sizeof(ProjTarget)), o_item = st.add(nitems * 4),
                 o_pq = st.add(nitems * sizeof(orb_proj_query)), o_q = st.add(nitems * 32);
    struct Regions {
        TrainStage train;
        size_t o_inv;
    };
    std::vector<Regions> tab;
    tab.reserve(nused);
    for (int k = 0; k < ntargets; k++) {
        const ProjView& V = targets[k];
        if (V.nq == 0 || V.side.n == 0) continue;
        Regions R{TrainStage{V.side, fuse && V.side.has_ur()}, 0};
        R.train.add_arrays(st, false);
        if (fuse) R.o_inv = st.add((size_t)V.nlevels * 4);
        R.train.add_grid(st);
        tab.push_back(R);
    }
    const size_t o_in_end = st.off;
    const size_t o_idx = st.add(nitems * 4), o_dist = st.add(nitems * 4);
    const int rr = st.alloc();
    if (rr != ORB_OK) return rr;
    size_t item = 0, row = 0;
    for (int k = 0; k < ntargets; k++) {
        const ProjView& V = targets[k];
        if (V.nq == 0 || V.side.n == 0) continue;
        const Regions& R = tab[row];
        ProjTarget& D = st.hi<ProjTarget>(o_tab)[row];
        D = R.train.row(st);
        D.inv_sigma2 = st.di<float>(R.o_inv);
        for (int i = 0; i < V.nq; i++) st.hi<int>(o_item)[item + i] = (int)row;
        std::memcpy(st.hi<orb_proj_query>(o_pq) + item, V.q, (size_t)V.nq * sizeof(orb_proj_query));
        std::memcpy(st.hi<uint8_t>(o_q) + item * 32, V.qdesc, (size_t)V.nq * 32);
        if (fuse) st.put(R.o_inv, V.inv_sigma2, (size_t)V.nlevels * 4);
        R.train.put(st);
        item += (size_t)V.nq;
        row++;
    }
    hipError_t e;
    if ((e = st.up(0, o_in_end)) != hipSuccess) return set_error("upload", e), ORB_ERR_HIP;
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 1, c->stream);
    e = launch_projection_best(gate, st.di<ProjTarget>(o_tab), st.di<int>(o_item), st.di<orb_proj_query>(o_pq),
                               st.di<uint8_t>(o_q), (int)nitems, st.h<int>(o_idx), st.h<int>(o_dist), c->stream);
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 0, c->stream);
    if (e != hipSuccess) return set_error("projection kernel", e), ORB_ERR_HIP;
    // the kernel writes (idx, dist) straight into the pinned mirror (host-coherent memory): no D2H command
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return set_error("download", e), ORB_ERR_HIP;
    item = 0;
    for (int k = 0; k < ntargets; k++) {
        const ProjView& V = targets[k];
        if (V.nq == 0 || V.side.n == 0) continue;
        std::memcpy(V.best_idx, st.h<int>(o_idx) + item, (size_t)V.nq * 4);
        std::memcpy(V.best_dist, st.h<int>(o_dist) + item, (size_t)V.nq * 4);
        item += (size_t)V.nq;
    }
    return ORB_OK;
}
}  // namespace
}  // namespace orbgpu

extern "C" {

/* Fuse (both overloads) and SearchBySim3's two directions: per (target, query) the first minimum of the descriptor
 * distance over the gated candidates, every target's items in one k_projection_best launch (orbgpu.h). */
int orb_project_best_batch(orb_ctx* h, int gate, int ntargets, const orb_proj_target* targets) {
    const char* const fn = "orb_project_best_batch";
    if (gate != ORB_PROJ_GATE_NONE && gate != ORB_PROJ_GATE_FUSE) return arg_error(fn, "unknown gate");
    if (ntargets < 0 || (ntargets > 0 && !targets)) return arg_error(fn, "ntargets < 0 or targets NULL");
    std::vector<ProjView> v;
    v.reserve(ntargets);
    for (int k = 0; k < ntargets; k++) v.push_back(proj_view(targets[k]));
    return project_best_run(fn, h, gate, v);
}

/* The same with every target's trains as a resident frame. */
int orb_project_best_frames(orb_ctx* h, int gate, int ntargets, const orb_proj_frame_target* targets) {
    const char* const fn = "orb_project_best_frames";
    if (gate != ORB_PROJ_GATE_NONE && gate != ORB_PROJ_GATE_FUSE) return arg_error(fn, "unknown gate");
    if (ntargets < 0 || (ntargets > 0 && !targets)) return arg_error(fn, "ntargets < 0 or targets NULL");
    std::vector<ProjView> v;
    v.reserve(ntargets);
    for (int k = 0; k < ntargets; k++) {
        if (!targets[k].frame) return arg_error(fn, "target " + std::to_string(k) + ": NULL frame");
        v.push_back(proj_view(targets[k]));
    }
    return project_best_run(fn, h, gate, v);
}

/* The grid searches with the train side as a resident frame (orbgpu.h): the frame's own checks, then the body the
 * host-pointer form runs, with the handle's device pointers and its host keypoints. */
int orb_search_by_projection_frame(orb_ctx* h, int mode, float nnratio, int check_ori, int max_dist, int nq,
                                   const orb_proj_query* q, const uint8_t* qdesc, const orb_frame* F,
                                   const uint8_t* t_taken, int use_uright, int* match_t, int* nmatches_out) {
    const char* const fn = "orb_search_by_projection_frame";
    if (const char* why = proj_scalars_fault(mode, max_dist)) return arg_error(fn, why);
    if (!F) return arg_error(fn, "NULL frame");
    if (nq < 0 || (F->n && !match_t) || (nq && (!q || !qdesc))) return arg_error(fn, "bad arguments");
    if (use_uright && !F->has_ur) return arg_error(fn, "use_uright with a frame created without uright");
    return projection_search_run(fn, h, mode, nnratio, check_ori, max_dist, nq, q, qdesc,
                                 TrainSide(F, use_uright != 0), t_taken, match_t, nmatches_out);
}

int orb_window_match_frame(orb_ctx* h, float nnratio, int check_ori, int level0_only, int n1, const uint8_t* desc1,
                           const orb_keypoint* kps1, const float* centres, float window, const orb_frame* F2,
                           int* match12, int* nmatches_out) {
    const char* const fn = "orb_window_match_frame";
    if (!F2) return arg_error(fn, "NULL frame");
    if (n1 < 0 || !match12 || (n1 && (!desc1 || !kps1))) return arg_error(fn, "bad arguments");
    return window_grid_run(fn, h, nnratio, check_ori, level0_only, n1, desc1, kps1, centres, window,
                           TrainSide(F2, false), match12, nmatches_out);
}

int orb_search_by_match_bird_resident(orb_ctx* h, float nnratio, int check_ori, int max_dist, float r, int nq,
                                      const int* q_id, const float* q_xy, const float* q_angle, const uint8_t* qdesc,
                                      const orb_frame* F, int* match_t, int* nmatches_out) {
    const char* const fn = "orb_search_by_match_bird_resident";
    if (const char* why = bird_scalars_fault(max_dist, r)) return arg_error(fn, why);
    if (!F) return arg_error(fn, "NULL frame");
    if (nq < 0 || (F->n && !match_t) || (nq && (!q_xy || !qdesc || (check_ori && !q_angle))))
        return arg_error(fn, "bad arguments");
    return match_bird_run(fn, h, nnratio, check_ori, max_dist, r, nq, q_id, q_xy, q_angle, qdesc, TrainSide(F, false),
                          match_t, nmatches_out);
}

int orb_project_best_host(int gate, const orb_proj_target* target, int query, int* best_idx, int* best_dist) {
    const char* const fn = "orb_project_best_host";
    if (gate != ORB_PROJ_GATE_NONE && gate != ORB_PROJ_GATE_FUSE) return arg_error(fn, "unknown gate");
    if (!target || !best_idx || !best_dist || query < 0 || query >= target->nq) return arg_error(fn, "bad arguments");
    orb_proj_target T = *target;   // (the target's own outputs are not this call's: not required, not touched)
    T.best_idx = best_idx;
    T.best_dist = best_dist;
    if (const char* why = proj_target_fault(gate, proj_view(T), query, query + 1)) return arg_error(fn, why);
    proj_best_one(gate, T, T.q[query], T.qdesc + (size_t)query * 32, best_idx, best_dist);
    return ORB_OK;
}

/* Frame::GetFeaturesInArea over the Frame grid (Frame.cc:378-392, 494-560) */
int orb_features_in_area(int n, const orb_keypoint* kps_un, float mnMinX, float mnMaxX, float mnMinY, float mnMaxY,
                         float x, float y, float r, int minLevel, int maxLevel, int* out, int cap) {
    const int COLS = kFrameGridCols, ROWS = kFrameGridRows;
    const float gw = static_cast<float>(COLS) / static_cast<float>(mnMaxX - mnMinX);
    const float gh = static_cast<float>(ROWS) / static_cast<float>(mnMaxY - mnMinY);
    std::vector<std::vector<int>> grid((size_t)COLS * ROWS);
    for (int i = 0; i < n; i++) {
        const int px = (int)std::round((kps_un[i].x - mnMinX) * gw);
        const int py = (int)std::round((kps_un[i].y - mnMinY) * gh);
        if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
        grid[(size_t)px * ROWS + py].push_back(i);
    }
    int cnt = 0;
    const CellRect c = cell_rect(x, y, r, mnMinX, mnMinY, gw, gh);
    if (c.empty) return 0;
    for (int ix = c.x0; ix <= c.x1; ix++)
        for (int iy = c.y0; iy <= c.y1; iy++)
            for (int idx : grid[(size_t)ix * ROWS + iy]) {
                if (!window_admits(kps_un[idx], x, y, r, minLevel, maxLevel)) continue;
                if (cnt < cap && out) out[cnt] = idx;
                cnt++;
            }
    return cnt > cap ? -cnt - 1 : cnt;
}

}  // extern "C"

namespace orbgpu {
namespace {

// What is wrong with target k of orb_fuse_search_points, or NULL.  k_projection_best indexes inv_sigma2 by the
// train's octave and k_project_points the slots by ids, so both are checked here.
const char* fuse_points_target_fault(const orb_points* P, const orb_fuse_points_target& T) {
    if (const char* why = camera_fault(&T.camera)) return why;
    if (const char* why = frustum_scalars_fault(0.0f, T.th)) return why;
    if (const char* why = point_ids_fault(P, T.n, T.ids)) return why;
    if (!T.frame) return "NULL frame";
    if (T.n > 0 && (!T.best_idx || !T.best_dist)) return "NULL outputs";
    if (!T.inv_sigma2) return "inv_sigma2 NULL";
    if (T.frame->n > 0 && (T.frame->oct_min < 0 || T.frame->oct_max >= T.camera.nlevels))
        return "train octave outside [0, nlevels)";
    return nullptr;
}

}  // namespace
}  // namespace orbgpu

extern "C" {

/* Tracking::SearchLocalPoints' isInFrustum loop and SearchByProjection(Frame&, vector<MapPoint*>, th) over resident
 * points and a resident frame (orbgpu.h): k_project_points, k_projection_topk and proj_replay, one synchronisation. */
int orb_search_local_points(orb_ctx* h, const orb_points* P, const orb_camera* camera, float view_cos_limit, float th,
                            float nnratio, int n, const int* ids, const orb_frame* F, const uint8_t* t_taken,
                            int use_uright, int* match_t, int* nmatches_out, orb_point_proj* proj_out) {
    const char* const fn = "orb_search_local_points";
    if (const char* why = camera_fault(camera)) return arg_error(fn, why);
    if (const char* why = frustum_scalars_fault(view_cos_limit, th)) return arg_error(fn, why);
    if (const char* why = point_ids_fault(P, n, ids)) return arg_error(fn, why);
    if (!F) return arg_error(fn, "NULL frame");
    if (F->n && !match_t) return arg_error(fn, "bad arguments");
    if (use_uright && !F->has_ur) return arg_error(fn, "use_uright with a frame created without uright");
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (c && P->device != c->device) return arg_error(fn, "the points live on another device");
    const TrainSide side(F, use_uright != 0);
    if (const int st = side_guard(fn, c, side)) return st;
    for (int t = 0; t < side.n; t++) match_t[t] = -1;
    if (nmatches_out) *nmatches_out = 0;
    if (n == 0 || side.n == 0) return ORB_OK;
    TopkSession s{c};
    int st = s.setup_points(P, point_cam(c, *camera, view_cos_limit, th), n, ids, side, proj_lanes(), proj_out != nullptr);
    if (st != ORB_OK) return st;
    // the replay reads a query's `blocks` only (RATIO_SAME_LEVEL): every map point here has observations (:87-89)
    std::vector<orb_proj_query> q((size_t)n, orb_proj_query{0.0f, 0.0f, 0.0f, -1, -1, 0.0f, 0.0f, 0.0f, 1});
    st = proj_replay(s, ORB_PROJ_RATIO_SAME_LEVEL, nnratio, 0, TH_HIGH, q.data(), side.kps, t_taken, match_t,
                     nmatches_out);
    if (st != ORB_OK) return st;
    if (proj_out) std::memcpy(proj_out, s.st.h<orb_point_proj>(s.o_rec), (size_t)n * sizeof(orb_point_proj));
    return ORB_OK;
}

/* Fuse(KeyFrame*, vector<MapPoint*>, th) for many keyframes over resident points and resident frames (orbgpu.h):
 * every target's items in one k_project_points launch (FUSE form, the item's camera) and one k_projection_best launch
 * (gate FUSE) over the queries it wrote. */
int orb_fuse_search_points(orb_ctx* h, const orb_points* P, int ntargets, const orb_fuse_points_target* targets) {
    const char* const fn = "orb_fuse_search_points";
    if (!P) return arg_error(fn, "NULL points handle");
    if (ntargets < 0 || (ntargets > 0 && !targets)) return arg_error(fn, "ntargets < 0 or targets NULL");
    size_t nitems = 0, nused = 0;
    bool want_rec = false;
    for (int k = 0; k < ntargets; k++) {
        const orb_fuse_points_target& T = targets[k];
        if (const char* why = fuse_points_target_fault(P, T))
            return arg_error(fn, "target " + std::to_string(k) + ": " + why);
        if (T.n > 0 && T.frame->n > 0) {
            nitems += (size_t)T.n;
            nused++;
            want_rec = want_rec || T.proj_out;
        }
    }
    if (nitems > (size_t)INT_MAX / 2) return arg_error(fn, "too many points");
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    if (P->device != c->device) return arg_error(fn, "the points live on another device");
    for (int k = 0; k < ntargets; k++)
        if (targets[k].frame->device != c->device)
            return arg_error(fn, "target " + std::to_string(k) + ": the frame lives on another device");
    CTX_GUARD(c);
    for (int k = 0; k < ntargets; k++)
        for (int i = 0; i < targets[k].n; i++) targets[k].best_idx[i] = targets[k].best_dist[i] = -1;
    if (nitems == 0) return ORB_OK;
    // staged and uploaded: [table | cameras | item -> row | ids | per used target inv_sigma2]; then the outputs, stored
    // into the mirror; past the mirror's end, device only: the queries and their descriptors (k_project_points' output)
    Stage st{c};
    const size_t o_tab = st.add(nused * sizeof(ProjTarget)), o_cam = st.add(nused * sizeof(PointCam)),
                 o_item = st.add(nitems * 4), o_ids = st.add(nitems * 4);
    std::vector<size_t> o_inv;
    o_inv.reserve(nused);
    for (int k = 0; k < ntargets; k++)
        if (targets[k].n > 0 && targets[k].frame->n > 0) o_inv.push_back(st.add((size_t)targets[k].camera.nlevels * 4));
    const size_t o_in_end = st.off;
    const size_t o_idx = st.add(nitems * 4), o_dist = st.add(nitems * 4),
                 o_rec = st.add(want_rec ? nitems * sizeof(orb_point_proj) : 0);
    st.end_mirror();
    const size_t o_pq = st.add(nitems * sizeof(orb_proj_query)), o_q = st.add(nitems * 32);
    const int rr = st.alloc();
    if (rr != ORB_OK) return rr;
    size_t item = 0, row = 0;
    for (int k = 0; k < ntargets; k++) {
        const orb_fuse_points_target& T = targets[k];
        if (T.n == 0 || T.frame->n == 0) continue;
        const TrainStage train{TrainSide(T.frame, true), T.frame->has_ur};
        ProjTarget& D = st.hi<ProjTarget>(o_tab)[row];
        D = train.row(st);
        D.inv_sigma2 = st.d<float>(o_inv[row]);
        st.hi<PointCam>(o_cam)[row] = point_cam(c, T.camera, 0.0f, T.th);
        for (int i = 0; i < T.n; i++) st.hi<int>(o_item)[item + i] = (int)row;
        std::memcpy(st.hi<int>(o_ids) + item, T.ids, (size_t)T.n * 4);
        st.put(o_inv[row], T.inv_sigma2, (size_t)T.camera.nlevels * 4);
        item += (size_t)T.n;
        row++;
    }
    hipError_t e;
    if ((e = st.up(0, o_in_end)) != hipSuccess) return set_error("upload", e), ORB_ERR_HIP;
    if ((e = launch_project_points(ORB_FRUSTUM_FUSE, st.d<PointCam>(o_cam), st.d<int>(o_item), st.d<int>(o_ids),
                                   (int)nitems, P->d_geo, P->d_desc,
                                   want_rec ? st.h<orb_point_proj>(o_rec) : nullptr, st.d<orb_proj_query>(o_pq),
                                   st.d<uint8_t>(o_q), c->stream)) != hipSuccess)
        return set_error("k_project_points", e), ORB_ERR_HIP;
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 1, c->stream);
    e = launch_projection_best(ORB_PROJ_GATE_FUSE, st.d<ProjTarget>(o_tab), st.d<int>(o_item),
                               st.d<orb_proj_query>(o_pq), st.d<uint8_t>(o_q), (int)nitems, st.h<int>(o_idx),
                               st.h<int>(o_dist), c->stream);
    if (c->prof_on) Ctx::marker(c, ORB_K_HAMMING, 0, c->stream);
    if (e != hipSuccess) return set_error("projection kernel", e), ORB_ERR_HIP;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return set_error("download", e), ORB_ERR_HIP;
    item = 0;
    for (int k = 0; k < ntargets; k++) {
        const orb_fuse_points_target& T = targets[k];
        if (T.n == 0 || T.frame->n == 0) continue;
        std::memcpy(T.best_idx, st.h<int>(o_idx) + item, (size_t)T.n * 4);
        std::memcpy(T.best_dist, st.h<int>(o_dist) + item, (size_t)T.n * 4);
        if (T.proj_out)
            std::memcpy(T.proj_out, st.h<orb_point_proj>(o_rec) + item, (size_t)T.n * sizeof(orb_point_proj));
        item += (size_t)T.n;
    }
    return ORB_OK;
}

}  // extern "C"
