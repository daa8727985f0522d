// gfx950 Hamming-distance kernels for ORBmatcher's vocabulary-gated searches (ORBmatcher.cc): the 256-bit
// distance (DescriptorDistance, ORBmatcher.cc:1647-1663) as 8 x (v_xor_b32 + v_bcnt_u32_b32) per pair on the VALU,
// over CSR candidate lists (k_topk), the Frame grid's windows (k_window_topk: one window size and the query's own
// level; k_projection_topk: per-query centre, radius, level range and stereo gate; k_projection_best: the first
// minimum per projected point over many keyframes' grids, with Fuse's reprojection gate) and SearchForTriangulation's
// epipolar-gated candidates (k_triangulation).  The all-pairs top-2 on the matrix cores is hamming_top2.hip.
// The selection logic that depends on the order of earlier accepted matches (SearchByBoW's taken set,
// SearchForInitialization's vMatchedDistance) is replayed on the host from these exact top-k lists
// (matcher.hip).
#include <algorithm>

#include "grid_window.h"
#include "orbgpu_internal.h"
#include "tri_geometry.h"

namespace orbgpu {

namespace {

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// minimum / sum over a row of W lanes (64: the wavefront; 16: one DPP row, the shuffles stay below lane offset 16)
template <int W>
__device__ __forceinline__ unsigned long long row_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) { return row_min_u64<64>(v); }
template <int W>
__device__ __forceinline__ int row_sum(int v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int kMaxK = 8;

// The top-k list of k_topk, k_window_topk and k_projection_topk: each lane keeps the k smallest keys it saw, ascending
// (key = dist << 32 | the candidate's rank in the reference's iteration order: ascending key = ascending distance,
// then first wins on ties); emit() merges the lanes' lists of a row of W lanes.  In registers: every index into lst
// is a constant after unrolling.
struct TopkList {
    unsigned long long lst[kMaxK];

    __device__ __forceinline__ TopkList() {
#pragma unroll
        for (int j = 0; j < kMaxK; j++) lst[j] = ~0ull;
    }

    __device__ __forceinline__ void insert(unsigned long long key, int k) {
#pragma unroll
        for (int j = 0; j < kMaxK; j++) {   // sorted insert (compare-swap chain)
            if (j < k && key < lst[j]) {
                const unsigned long long tmp = lst[j];
                lst[j] = key;
                key = tmp;
            }
        }
    }

    // The row's k smallest keys in order: k times the minimum of the lanes' heads, the lane that holds it steps on
    // (keys are unique within a row).  The writer lane (one per row, or none) stores entry j of out_dist / out_idx
    // at row * k + j: the key's distance and idx_of(its low word), or -1, -1 once the row's lists are exhausted.
    // Every lane of the row must call (shuffles).
    template <int W, class IdxOf>
    __device__ __forceinline__ void emit(int k, bool writer, long long row, IdxOf idx_of, int* __restrict__ out_dist,
                                         int* __restrict__ out_idx) const {
        int head = 0;
        for (int j = 0; j < k; j++) {
            unsigned long long mine = ~0ull;
#pragma unroll
            for (int s = 0; s < kMaxK; s++)
                if (s == head) mine = lst[s];
            const unsigned long long m = row_min_u64<W>(mine);
            if (mine == m && m != ~0ull) head++;
            if (writer) {
                int dd = -1, ii = -1;
                if (m != ~0ull) {
                    dd = (int)(m >> 32);
                    ii = idx_of((int)(m & 0xFFFFFFFFu));
                }
                out_dist[row * k + j] = dd;
                out_idx[row * k + j] = ii;
            }
        }
    }
};

}  // namespace

/* Top-k per query over a CSR candidate list (or all trains), one wavefront per query.
 * Key = dist << 32 | candidate position: ascending key = ascending distance, then the reference's
 * iteration order (first wins on ties, as the strict '<' updates of ORBmatcher.cc:216-225 do). */
__global__ __launch_bounds__(256) void k_topk(const uint8_t* __restrict__ q, int nq, const uint8_t* __restrict__ t,
                                              int nt, const int2* __restrict__ ranges,
                                              const int* __restrict__ cand_idx, const int* __restrict__ thr, int k,
                                              int* __restrict__ out_dist, int* __restrict__ out_idx,
                                              int* __restrict__ out_nvalid) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (qi >= nq) return;
    const uint4* qp = reinterpret_cast<const uint4*>(q + (long long)qi * 32);
    const uint4 qa = qp[0], qb = qp[1];
    int c0 = 0, c1 = nt;
    if (ranges) {
        const int2 r = ranges[qi];
        c0 = r.x;
        c1 = r.y;
    }
    TopkList top;
    int nvalid = 0;
    for (int pos = c0 + lane; pos < c1; pos += 64) {
        const int ti = ranges ? cand_idx[pos] : pos;
        const uint4* tp = reinterpret_cast<const uint4*>(t + (long long)ti * 32);
        const int d = hamming256(qa, qb, tp[0], tp[1]);
        if (thr && thr[ti] <= d) continue;
        nvalid++;
        top.insert(((unsigned long long)d << 32) | (unsigned)(pos - c0), k);
    }
    nvalid = row_sum<64>(nvalid);
    top.emit<64>(k, lane == 0, qi, [&](int rank) { return ranges ? cand_idx[rank + c0] : rank + c0; }, out_dist, out_idx);
    if (lane == 0 && out_nvalid) out_nvalid[qi] = nvalid;
}

// The window searches' candidate lists built on the device (SearchForInitialization :416-437,
// BirdviewMatch :1680-1700 / :1801-1812): Frame::GetFeaturesInArea(cx, cy, r, lv, lv) with lv = the
// query's octave (:494-547; the rectangle and the box are grid_window.h's) over F2's grid in its CSR form.  The
// reference visits cells ix-major, iy
// inner, a cell's keypoints in vector order: that is increasing CSR slot, so a candidate's slot is its
// rank in vIndices2 and (dist, slot) breaks ties as the reference's first minimum does.  One wave per
// item; the rectangle's column ranges are contiguous slot runs.
__global__ __launch_bounds__(256) void k_window_topk(const uint8_t* __restrict__ q, const int* __restrict__ item_q,
                                                     const float2* __restrict__ centre, int nitems,
                                                     const orb_keypoint* __restrict__ kps1,
                                                     const uint8_t* __restrict__ t,
                                                     const orb_keypoint* __restrict__ kps2,
                                                     const int* __restrict__ cell_off,
                                                     const int* __restrict__ cell_idx, WinGrid wg,
                                                     const int* __restrict__ thr, int k, int* __restrict__ out_dist,
                                                     int* __restrict__ out_idx, int* __restrict__ out_nvalid) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (qi >= nitems) return;
    const int i1 = item_q[qi];
    const uint4* qp = reinterpret_cast<const uint4*>(q + (long long)i1 * 32);
    const uint4 qa = qp[0], qb = qp[1];
    const int lv = kps1[i1].octave;
    float x, y;
    if (centre) {
        const float2 cc = centre[i1];
        x = cc.x;
        y = cc.y;
    } else {
        x = kps1[i1].x;
        y = kps1[i1].y;
    }
    const float r = wg.r;
    const CellRect c = cell_rect(x, y, r, wg.min_x, wg.min_y, wg.inv_w, wg.inv_h);
    TopkList top;
    int nvalid = 0;
    if (!c.empty) {
        for (int ix = c.x0; ix <= c.x1; ix++) {
            const int s0 = cell_off[ix * kCellGridRows + c.y0], s1 = cell_off[ix * kCellGridRows + c.y1 + 1];
            for (int s = s0 + lane; s < s1; s += 64) {
                const int ti = cell_idx[s];
                const orb_keypoint kp = kps2[ti];
                if (kp.octave != lv) continue;   // the query's own level (grid_window.h on why not window_admits)
                if (!window_box(kp, x, y, r)) continue;
                const uint4* tp = reinterpret_cast<const uint4*>(t + (long long)ti * 32);
                const int d = hamming256(qa, qb, tp[0], tp[1]);
                if (thr && thr[ti] <= d) continue;
                nvalid++;
                top.insert(((unsigned long long)d << 32) | (unsigned)s, k);
            }
        }
    }
    nvalid = row_sum<64>(nvalid);
    top.emit<64>(k, lane == 0, qi, [&](int slot) { return cell_idx[slot]; }, out_dist, out_idx);
    if (lane == 0 && out_nvalid) out_nvalid[qi] = nvalid;
}

// The projection-gated searches' candidates (SearchByProjection(Frame&, const Frame&) :1383-1413,
// SearchByProjection(Frame&, vector<MapPoint*>) :68-96, SearchByProjectionBird :1945-1965):
// Frame::GetFeaturesInArea(u, v, r, min_level, max_level) (Frame.cc:494-547: cell_rect and window_admits,
// grid_window.h) over the train frame's grid in its CSR form, each query with its own centre, radius and level range, then the stereo gate on mvuRight.  As in
// k_window_topk a candidate's CSR slot is its rank in vIndices, so (dist, slot) is the reference's first minimum.
// A projection window holds a few to a few dozen candidates; a query gets W lanes: 64 (one wavefront, the form in
// use) or 16 (one DPP row: four queries per wavefront, sixteen per block; the reductions stay below lane offset 16;
// measured no faster, DESIGN 5.3, and kept for that A/B).
// Rows of a wavefront whose query index is past nq stay in the kernel with an empty window, so every shuffle
// runs with all of its row's lanes active.
template <int W>
__global__ __launch_bounds__(256) void k_projection_topk(const orb_proj_query* __restrict__ pq,
                                                         const uint8_t* __restrict__ q, int nq,
                                                         const uint8_t* __restrict__ t,
                                                         const orb_keypoint* __restrict__ kps2,
                                                         const float* __restrict__ uright,
                                                         const int* __restrict__ cell_off,
                                                         const int* __restrict__ cell_idx, ProjGrid g,
                                                         const int* __restrict__ thr, int k,
                                                         int* __restrict__ out_dist, int* __restrict__ out_idx,
                                                         int* __restrict__ out_nvalid) {
    static_assert(W == 16 || W == 64, "one DPP row or one wavefront per query");
    const int qi = blockIdx.x * (256 / W) + (int)(threadIdx.x / W);
    const int lane = threadIdx.x & (W - 1);
    const bool live = qi < nq;
    const int qc = live ? qi : nq - 1;   // (nq >= 1: the launcher returns before an empty launch)
    const orb_proj_query P = pq[qc];
    const uint4* qp = reinterpret_cast<const uint4*>(q + (long long)qc * 32);
    const uint4 qa = qp[0], qb = qp[1];
    const float x = P.u, y = P.v, r = P.r;
    const CellRect c = cell_rect(x, y, r, g.min_x, g.min_y, g.inv_w, g.inv_h);
    TopkList top;
    int nvalid = 0;
    if (live && !c.empty) {
        for (int ix = c.x0; ix <= c.x1; ix++) {
            const int s0 = cell_off[ix * kCellGridRows + c.y0], s1 = cell_off[ix * kCellGridRows + c.y1 + 1];
            for (int s = s0 + lane; s < s1; s += W) {
                const int ti = cell_idx[s];
                const orb_keypoint kp = kps2[ti];
                if (!window_admits(kp, x, y, r, P.min_level, P.max_level)) continue;
                if (uright) {                                                         // ORBmatcher.cc:91-96, :1407-1413
                    const float urt = uright[ti];
                    if (urt > 0 && fabsf(P.ur - urt) > P.ur_tol) continue;
                }
                const uint4* tp = reinterpret_cast<const uint4*>(t + (long long)ti * 32);
                const int d = hamming256(qa, qb, tp[0], tp[1]);
                if (thr && thr[ti] <= d) continue;
                nvalid++;
                top.insert(((unsigned long long)d << 32) | (unsigned)s, k);
            }
        }
    }
    nvalid = row_sum<W>(nvalid);
    top.emit<W>(k, lane == 0 && live, qi, [&](int slot) { return cell_idx[slot]; }, out_dist, out_idx);
    if (lane == 0 && live) out_nvalid[qi] = nvalid;
}

// The searches that decide every projected point on its own: Fuse(KeyFrame*, vector<MapPoint*>, th) (:892-949,
// GATE 1), Fuse(KeyFrame*, Scw, ...) (:1051-1079) and both directions of SearchBySim3 (:1191-1219, :1271-1299)
// (GATE 0).  One wavefront per (target, query) item, the items of all targets in one launch; the item's target row
// gives where its keyframe's descriptors, keypoints, mvuRight, mvInvLevelSigma2 and grid CSR lie (device pointers:
// the call's staging area, or a resident frame).  The walk is k_projection_topk's (KeyFrame::GetFeaturesInArea is
// Frame::GetFeaturesInArea without levels; the level filter of the callers is the query's (min_level, max_level));
// a lane keeps one key dist << 32 | slot (a slot is the candidate's rank in vIndices), so the wave minimum is the
// reference's first minimum.
// GATE 1: the chi-square reprojection test of :914-938, fuse_gate_skips (grid_window.h: the reference build's
// contracted forms; this file builds -ffp-contract=off, so its fmaf are the only fused operations); the octave
// indexes inv_sigma2, which the host validated.  Waves past the last item stay in with an empty window.
template <int GATE>
__global__ __launch_bounds__(256) void k_projection_best(const ProjTarget* __restrict__ tab,
                                                         const int* __restrict__ item_tgt,
                                                         const orb_proj_query* __restrict__ pq,
                                                         const uint8_t* __restrict__ q, int nitems,
                                                         int* __restrict__ out_idx, int* __restrict__ out_dist) {
    const int it = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool live = it < nitems;
    const int ic = live ? it : nitems - 1;   // (nitems >= 1: the launcher returns before an empty launch)
    const orb_proj_query P = pq[ic];
    const ProjTarget T = tab[item_tgt[ic]];
    const uint4* qp = reinterpret_cast<const uint4*>(q + (long long)ic * 32);
    const uint4 qa = qp[0], qb = qp[1];
    const uint8_t* t = T.t;
    const orb_keypoint* kps = T.kps;
    const float* uright = T.ur;
    const float* inv_sigma2 = T.inv_sigma2;
    const int* cell_off = T.cell_off;
    const int* cell_idx = T.cell_idx;
    const ProjGrid g = T.g;
    const float x = P.u, y = P.v, r = P.r;
    const CellRect c = cell_rect(x, y, r, g.min_x, g.min_y, g.inv_w, g.inv_h);
    unsigned long long best = ~0ull;
    if (live && !c.empty) {
        for (int ix = c.x0; ix <= c.x1; ix++) {
            const int s0 = cell_off[ix * kCellGridRows + c.y0], s1 = cell_off[ix * kCellGridRows + c.y1 + 1];
            for (int s = s0 + lane; s < s1; s += 64) {
                const int ti = cell_idx[s];
                const orb_keypoint kp = kps[ti];
                if (!window_admits(kp, x, y, r, P.min_level, P.max_level)) continue;
                if (GATE == ORB_PROJ_GATE_FUSE &&
                    fuse_gate_skips(x, y, P.ur, kp.x, kp.y, uright ? uright[ti] : -1.0f, inv_sigma2[kp.octave]))
                    continue;
                const uint4* tp = reinterpret_cast<const uint4*>(t + (long long)ti * 32);
                const int d = hamming256(qa, qb, tp[0], tp[1]);
                const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)s;
                best = key < best ? key : best;
            }
        }
    }
    best = wave_min_u64(best);
    if (lane == 0 && live) {
        int dd = -1, ii = -1;
        if (best != ~0ull) {
            dd = (int)(best >> 32);
            ii = cell_idx[(int)(best & 0xFFFFFFFFu)];
        }
        out_idx[it] = ii;
        out_dist[it] = dd;
    }
}

/* SearchForTriangulation inner loop (ORBmatcher.cc:712-761) for one (idx1, node) item per
 * wavefront: dist <= TH_LOW, epipole distance gate for mono pairs, CheckDistEpipolarLine
 * (:140-157, float with the final comparison in double).  The reference keeps the LAST candidate
 * reaching the running minimum ('dist > bestDist' skips only strictly larger), so the key is
 * dist << 32 | ~pos.  The inputs live in host memory (the call's pinned mirror): the item record is one
 * wave-uniform read, then each lane reads its candidates' records. */
__global__ __launch_bounds__(256) void k_triangulation(const TriItem* __restrict__ items,
                                                       const TriTrain* __restrict__ trains, int nitems,
                                                       int* __restrict__ best_out) {
    const int it = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (it >= nitems) return;
    const TriItem q = items[it];
    const bool st1 = q.stereo != 0;
    // CheckDistEpipolarLine (tri_epipolar_ok, tri_geometry.h): the line a, b, c comes staged with the query
    const float la = q.la, lb = q.lb, lc = q.lc;
    const float den = __builtin_fmaf(la, la, lb * lb);
    unsigned long long bestKey = ~0ull;
    const int c0 = q.c0, c1 = q.c1;
    for (int pos = c0 + lane; pos < c1; pos += 64) {
        const TriTrain& tr = trains[pos];   // (no map point, stereo if asked: filtered on the host, :725-733)
        const uint4 ta = tr.desc[0], tb = tr.desc[1];
        const int dist = hamming256(q.desc[0], q.desc[1], ta, tb);
        if (dist > 50) continue;
        const int fl = tr.flags;
        if (!st1 && !(fl & 1) && (fl & 2)) continue;   // neither stereo and too close to the epipole (:743-748)
        // (den is the item's, wave-uniform: tested here as well, ahead of the record's loads from the host mirror, the
        // function's own test folds away; without this line the loop gains a scalar branch and measured slower)
        if (den == 0) continue;
        if (!tri_epipolar_ok(la, lb, lc, den, tr.x, tr.y, tr.sigma2)) continue;
        const unsigned long long key = ((unsigned long long)dist << 32) | (unsigned)(0x7FFFFFFF - (pos - c0));
        bestKey = key < bestKey ? key : bestKey;
    }
    bestKey = wave_min_u64(bestKey);
    if (lane == 0) best_out[it] = bestKey != ~0ull ? c0 + (0x7FFFFFFF - (int)(bestKey & 0xFFFFFFFFu)) : -1;
}

/* SearchForTriangulation (ORBmatcher.cc:684-761) between two resident frames, one wavefront per (pair, KF1 feature):
 * the feature's node is looked up in KF2's FeatureVector (a wave-uniform binary search), the lanes stride the node's
 * candidates in CSR order, and the pair's float work (tri_geometry.h) runs here instead of on staged records.  The
 * tests and the key are k_triangulation's; a candidate's position is its place in the node's CSR order (the host
 * form numbers the candidates that pass the map-point / stereo filter, in the same order: the same winner).
 * Reads: node_of / has_mp / ur / kps / desc of KF1 at idx1 < n1; fv_nodes[0, nnodes), fv_off[0, nnodes], fv_idx below
 * fv_off[nnodes]; KF2's arrays at fv_idx's entries (< n2, featvec_ok or k_frame_featvec); scale2 / sigma2 at a KF2
 * octave (the host checked the frame's octaves against nlevels2).  Writes best_out[pair * n1 + idx1]. */
__global__ __launch_bounds__(256) void k_triangulation_frames(TriFrameKf1 A, const TriFramePair* __restrict__ tab,
                                                              int only_stereo, int* __restrict__ best_out) {
    const int idx1 = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (idx1 >= A.n) return;
    const int p = blockIdx.y;
    int* const out = best_out + (long long)p * A.n + idx1;
    const uint32_t nd = A.node_of[idx1];
    const bool st1 = A.ur[idx1] >= 0;
    // a map point already (:694-696), outside KF1's FeatureVector, or mono under bOnlyStereo (:698-702)
    if (A.has_mp[idx1] || nd == 0xFFFFFFFFu || (only_stereo && !st1)) {
        if (lane == 0) *out = -1;
        return;
    }
    const TriFramePair& P = tab[p];
    int lo = 0, hi = P.nnodes;   // the first node of KF2 not below nd
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (P.fv_nodes[mid] < nd) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= P.nnodes || P.fv_nodes[lo] != nd) {
        if (lane == 0) *out = -1;
        return;
    }
    const int c0 = P.fv_off[lo], c1 = P.fv_off[lo + 1];
    const uint4* qp = reinterpret_cast<const uint4*>(A.desc + (long long)idx1 * 32);
    const uint4 qa = qp[0], qb = qp[1];
    const orb_keypoint k1 = A.kps[idx1];
    float la, lb, lc;
    tri_line(k1.x, k1.y, P.F, la, lb, lc);
    const float den = __builtin_fmaf(la, la, lb * lb);
    unsigned long long bestKey = ~0ull;
    for (int pos = c0 + lane; pos < c1; pos += 64) {
        const int i2 = P.fv_idx[pos];
        if (P.has_mp[i2]) continue;                    // :725-727
        const bool st2 = P.ur[i2] >= 0;
        if (only_stereo && !st2) continue;             // :729-733
        const uint4* tp = reinterpret_cast<const uint4*>(P.desc + (long long)i2 * 32);
        const int dist = hamming256(qa, qb, tp[0], tp[1]);
        if (dist > 50) continue;
        const orb_keypoint& k2 = P.kps[i2];
        const float x2 = k2.x, y2 = k2.y;
        const int oct = k2.octave;
        if (!st1 && !st2 && tri_near_epipole(P.ex, P.ey, x2, y2, P.scale2, oct)) continue;   // :743-748
        if (!tri_epipolar_ok(la, lb, lc, den, x2, y2, tri_sigma2(P.sigma2, oct))) continue;
        const unsigned long long key = ((unsigned long long)dist << 32) | (unsigned)(0x7FFFFFFF - (pos - c0));
        bestKey = key < bestKey ? key : bestKey;
    }
    bestKey = wave_min_u64(bestKey);
    if (lane == 0) *out = bestKey != ~0ull ? P.fv_idx[c0 + (0x7FFFFFFF - (int)(bestKey & 0xFFFFFFFFu))] : -1;
}

/* The items of SearchByBoW between resident frames, one workgroup per keyframe of the batch: every position k of the
 * query side's FeatureVector CSR, in order (ascending node, then the node's order: the reference's iteration order),
 * is an item iff its node is also a node of the train side and the feature's flag is set.  The kept positions are
 * compacted in order (ballot + wave counts) to [seg0, seg0 + len); an item gets its feature index, its candidate range
 * in the train CSR and its descriptor, item-major, for k_topk.  The rest of the segment gets an empty range, so one
 * k_topk launch over every segment's capacity ranks nothing there.
 * Reads: q_off[0, q_nnodes], q_nodes / t_nodes below their counts, t_off[b + 1] with b < t_nnodes, q_idx[k] with
 * k < q_nnz, q_flag / q_desc at q_idx's entries.  Writes: the segment's q_nnz slots of the three arrays, seg_len[p]. */
__global__ __launch_bounds__(256) void k_bow_items(const BowItemsRow* __restrict__ tab, int* __restrict__ item_q,
                                                   int2* __restrict__ item_rng, uint8_t* __restrict__ qbuf,
                                                   int* __restrict__ seg_len) {
    __shared__ int s_wave[4];
    const BowItemsRow R = tab[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int done = 0;
    for (int k0 = 0; k0 < R.q_nnz; k0 += 256) {   // (uniform trip count)
        const int k = k0 + tid;
        bool keep = false;
        int feat = 0;
        int2 rng = make_int2(0, 0);
        if (k < R.q_nnz) {
            int lo = 0, hi = R.q_nnodes;   // the first node whose offset is above k (q_off[q_nnodes] = q_nnz > k)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (R.q_off[mid] <= k) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t nd = R.q_nodes[lo - 1];   // (q_off[0] = 0 <= k: lo >= 1)
            int b = 0, e = R.t_nnodes;
            while (b < e) {
                const int mid = (b + e) >> 1;
                if (R.t_nodes[mid] < nd) b = mid + 1;
                else e = mid;
            }
            feat = R.q_idx[k];
            if (b < R.t_nnodes && R.t_nodes[b] == nd && R.q_flag[feat]) {
                keep = true;
                rng = make_int2(R.rng_base + R.t_off[b], R.rng_base + R.t_off[b + 1]);
            }
        }
        const unsigned long long m = __ballot(keep);
        __syncthreads();   // the previous step's s_wave has been read
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int pos = done + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < 4; w++) {
            if (w < wave) pos += s_wave[w];
            total += s_wave[w];
        }
        if (keep) {   // pos < the number of kept positions <= q_nnz
            const long long o = (long long)R.seg0 + pos;
            item_q[o] = feat;
            item_rng[o] = rng;
            const uint4* src = reinterpret_cast<const uint4*>(R.q_desc + (long long)feat * 32);
            uint4* dst = reinterpret_cast<uint4*>(qbuf + o * 32);
            dst[0] = src[0];
            dst[1] = src[1];
        }
        done += total;
    }
    for (int k = done + tid; k < R.q_nnz; k += 256) item_rng[(long long)R.seg0 + k] = make_int2(0, 0);
    if (tid == 0) seg_len[blockIdx.x] = done;
}

hipError_t launch_triangulation_frames(const TriFrameKf1& a, const TriFramePair* d_tab, int npairs, int only_stereo,
                                       int* best_out, hipStream_t stream) {
    if (npairs <= 0 || a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_triangulation_frames, dim3((a.n + 3) / 4, npairs), dim3(256), 0, stream, a, d_tab, only_stereo,
                       best_out);
    return hipGetLastError();
}

hipError_t launch_bow_items(const BowItemsRow* d_tab, int nkf, int* item_q, int2* d_item_rng, uint8_t* d_qbuf,
                            int* seg_len, hipStream_t stream) {
    if (nkf <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bow_items, dim3(nkf), dim3(256), 0, stream, d_tab, item_q, d_item_rng, d_qbuf, seg_len);
    return hipGetLastError();
}

hipError_t launch_hamming_topk(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, const int2* d_ranges,
                               const int* d_cand_idx, const int* d_thr, int k, int* d_dist, int* d_idx, int* d_nvalid,
                               hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (k < 1 || k > kMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_topk, dim3((nq + 3) / 4), dim3(256), 0, stream, d_q, nq, d_t, nt, d_ranges, d_cand_idx,
                       d_thr, k, d_dist, d_idx, d_nvalid);
    return hipGetLastError();
}

hipError_t launch_window_topk(const uint8_t* d_q, const int* d_item_q, const float2* d_centre, int nitems,
                              const orb_keypoint* d_kps1, const uint8_t* d_t, const orb_keypoint* d_kps2,
                              const int* d_cell_off, const int* d_cell_idx, const WinGrid& wg, const int* d_thr,
                              int k, int* d_dist, int* d_idx, int* d_nvalid, hipStream_t stream) {
    if (nitems <= 0) return hipSuccess;
    if (k < 1 || k > kMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_window_topk, dim3((nitems + 3) / 4), dim3(256), 0, stream, d_q, d_item_q, d_centre, nitems,
                       d_kps1, d_t, d_kps2, d_cell_off, d_cell_idx, wg, d_thr, k, d_dist, d_idx, d_nvalid);
    return hipGetLastError();
}

hipError_t launch_projection_topk(const orb_proj_query* d_pq, const uint8_t* d_q, int nq, const uint8_t* d_t,
                                  const orb_keypoint* d_kps2, const float* d_uright, const int* d_cell_off,
                                  const int* d_cell_idx, const ProjGrid& g, const int* d_thr, int k, int lanes,
                                  int* d_dist, int* d_idx, int* d_nvalid, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (k < 1 || k > kMaxK || (lanes != 16 && lanes != 64)) return hipErrorInvalidValue;
    if (lanes == 16)
        hipLaunchKernelGGL(k_projection_topk<16>, dim3((nq + 15) / 16), dim3(256), 0, stream, d_pq, d_q, nq, d_t, d_kps2,
                           d_uright, d_cell_off, d_cell_idx, g, d_thr, k, d_dist, d_idx, d_nvalid);
    else
        hipLaunchKernelGGL(k_projection_topk<64>, dim3((nq + 3) / 4), dim3(256), 0, stream, d_pq, d_q, nq, d_t, d_kps2,
                           d_uright, d_cell_off, d_cell_idx, g, d_thr, k, d_dist, d_idx, d_nvalid);
    return hipGetLastError();
}

hipError_t launch_projection_best(int gate, const ProjTarget* d_tab, const int* d_item_tgt, const orb_proj_query* d_pq,
                                  const uint8_t* d_q, int nitems, int* d_idx, int* d_dist, hipStream_t stream) {
    if (nitems <= 0) return hipSuccess;
    if (gate == ORB_PROJ_GATE_FUSE)
        hipLaunchKernelGGL(k_projection_best<ORB_PROJ_GATE_FUSE>, dim3((nitems + 3) / 4), dim3(256), 0, stream,
                           d_tab, d_item_tgt, d_pq, d_q, nitems, d_idx, d_dist);
    else if (gate == ORB_PROJ_GATE_NONE)
        hipLaunchKernelGGL(k_projection_best<ORB_PROJ_GATE_NONE>, dim3((nitems + 3) / 4), dim3(256), 0, stream,
                           d_tab, d_item_tgt, d_pq, d_q, nitems, d_idx, d_dist);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_triangulation(const TriItem* d_items, const TriTrain* d_trains, int nitems, int* d_best,
                                hipStream_t stream) {
    if (nitems <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_triangulation, dim3((nitems + 3) / 4), dim3(256), 0, stream, d_items, d_trains, nitems, d_best);
    return hipGetLastError();
}

}  // namespace orbgpu
