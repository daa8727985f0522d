// The BoW part of a resident frame (orb_frame_bow, orbgpu_ctx.h): Frame::ComputeBoW / KeyFrame::ComputeBoW
// (Frame.cc:562-569, KeyFrame.cc:74-83) for handles, without the frame's descriptors or triples leaving the device.
// k_vocab_transform (vocab.hip) gives every feature its (word, weight, node); k_frame_featvec assembles each frame's
// FeatureVector (FeatureVector::addFeature, FeatureVector.cpp:31-45: a std::map of node id to the features in input
// order) as CSR.  The BowVector's double sums depend on their order and stay on the host (vocab_bow_vector).
#include <climits>
#include <cstring>
#include <new>

#include "orbgpu_ctx.h"

namespace orbgpu {

constexpr int kFvThreads = 1024;
constexpr int kFvWaves = kFvThreads / 64;

struct FeatvecRow {   // one frame of a k_frame_featvec launch
    const uint32_t* tnode;   // k_vocab_transform's node per feature
    const float* weight;
    int* meta;               // nnodes, nnz
    uint32_t* fv_nodes;
    int* fv_off;
    int* fv_idx;
    uint32_t* node_of;
    int n;
    int stopped_all;         // the vocabulary has no words: transform() returns empty vectors
};

// One frame per workgroup.  A feature is in the FeatureVector iff (double)weight > 0 (DBoW2's "not stopped"); its key
// is its node id, kBowNoNode otherwise (a vocabulary's node ids are below 2^27).
//   1. Rank: feature i's place in fv_idx is the number of features with a smaller (node, index) key; the keys are
//      distinct, so the places are a permutation of [0, nnz).  The keys pass through LDS in tiles of kFvThreads, every
//      thread counting a tile against its own key: n^2 / kFvThreads compares per thread and no bound on n.
//   2. Nodes: position p of fv_idx starts a node iff p == 0 or its node differs from position p - 1's; the starts are
//      compacted in order (ballot + wave counts, as k_frame_grid's long cells) into fv_nodes / fv_off.
// Writes: fv_idx[rank] with rank < nnz <= n; fv_nodes / fv_off[pos] with pos < nnodes <= nnz; fv_off[nnodes];
// node_of[i], i < n; meta[0..1].
__global__ __launch_bounds__(kFvThreads) void k_frame_featvec(const FeatvecRow* __restrict__ tab) {
    __shared__ uint32_t s_key[kFvThreads];
    __shared__ int s_wave[kFvWaves];
    __shared__ int s_nnz;
    const FeatvecRow R = tab[blockIdx.x];
    const int n = R.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_nnz = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += kFvThreads) {   // (uniform trip count: the barriers below are reached by all)
        const int i = i0 + tid;
        uint32_t key = kBowNoNode;
        if (i < n) {
            if (!R.stopped_all && (double)R.weight[i] > 0) key = R.tnode[i];
            R.node_of[i] = key;
        }
        int rank = 0;
        for (int j0 = 0; j0 < n; j0 += kFvThreads) {
            const int j = j0 + tid;
            __syncthreads();   // the previous tile has been read
            s_key[tid] = (j < n && !R.stopped_all && (double)R.weight[j] > 0) ? R.tnode[j] : kBowNoNode;
            __syncthreads();
            const int m = min(kFvThreads, n - j0);
            // keys before i in index order count on '<=', keys after on '<': ties (one node) order by index
            const int split = min(max(i - j0, 0), m);
            for (int k = 0; k < split; k++) rank += s_key[k] <= key;
            for (int k = split; k < m; k++) rank += s_key[k] < key;
        }
        if (key != kBowNoNode) {
            R.fv_idx[rank] = i;
            atomicAdd(&s_nnz, 1);
        }
    }
    __syncthreads();   // fv_idx is complete and read below by other threads of this workgroup
    const int nnz = s_nnz;
    int done = 0;
    for (int p0 = 0; p0 < nnz; p0 += kFvThreads) {
        const int p = p0 + tid;
        uint32_t nd = 0;
        bool start = false;
        if (p < nnz) {
            nd = R.tnode[R.fv_idx[p]];
            start = p == 0 || R.tnode[R.fv_idx[p - 1]] != nd;
        }
        const unsigned long long b = __ballot(start);
        __syncthreads();   // the previous step's s_wave has been read
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int pos = done + __popcll(b & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < kFvWaves; w++) {
            if (w < wave) pos += s_wave[w];
            total += s_wave[w];
        }
        if (start) {
            R.fv_nodes[pos] = nd;
            R.fv_off[pos] = p;
        }
        done += total;
    }
    if (tid == 0) {
        R.fv_off[done] = nnz;   // (done <= n: fv_off holds n + 1)
        R.meta[0] = done;
        R.meta[1] = nnz;
    }
}

namespace {

// A BoW part for n features, allocated on the current device with its host copy sized; NULL and e on failure.
orb_frame_bow* bow_alloc(int n, int ncap, int icap, bool triples, hipError_t& e) {
    orb_frame_bow* B = new (std::nothrow) orb_frame_bow();
    if (!B) return nullptr;
    B->L = bow_layout(n, ncap, icap, triples);
    B->triples = triples;
    if ((e = B->d_base.ensure(B->L.bytes)) != hipSuccess) {
        delete B;
        return nullptr;
    }
    try {
        B->h.assign(B->L.bytes, 0);
    } catch (const std::bad_alloc&) {
        delete B;
        return nullptr;
    }
    return B;
}

void bow_attach(orb_frame* F, orb_frame_bow* B) {
    delete F->bow;   // (the caller synchronised: nothing queued reads the old part)
    F->bow = B;
}

}  // namespace
}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_frame_compute_bow(orb_ctx* h, const orb_vocab* v, int levelsup, int nframes, orb_frame* const* frames) {
    const char* const fn = "orb_frame_compute_bow";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (nframes < 0) return arg_error(fn, "nframes < 0");
    if (nframes > 0 && !frames) return arg_error(fn, "frames NULL");
    if (!v) return arg_error(fn, "NULL vocabulary");
    for (int f = 0; f < nframes; f++) {
        if (!frames[f]) return arg_error(fn, "NULL frame");
        for (int g = 0; g < f; g++)
            if (frames[g] == frames[f]) return arg_error(fn, "a frame listed twice");
    }
    CTX_GUARD(c);
    if (vocab_device(v) != c->device) return arg_error(fn, "vocabulary of another device");
    for (int f = 0; f < nframes; f++)
        if (frames[f]->device != c->device) return arg_error(fn, "frame of another device");
    if (nframes == 0) return ORB_OK;
    hipError_t e = hipSuccess;
    std::vector<orb_frame_bow*> parts(nframes, nullptr);
    auto fail = [&](const char* what, int st) {
        set_error(what, e);
        (void)hipStreamSynchronize(c->stream);   // queued work writes into the parts: it ends before they are freed
        for (orb_frame_bow* B : parts) delete B;
        return st;
    };
    int max_n = 0;
    for (int f = 0; f < nframes; f++) {
        if (!(parts[f] = bow_alloc(frames[f]->n, frames[f]->n, frames[f]->n, true, e))) return fail("orb_frame_compute_bow: allocation", ORB_ERR_NOMEM);
        max_n = std::max(max_n, frames[f]->n);
    }
    // the two launches' tables, read from the pinned mirror (two small reads per workgroup)
    Stage st{c};
    st.zc = 1;
    const size_t o_vt = st.add((size_t)nframes * sizeof(VocabFrameRow)), o_ft = st.add((size_t)nframes * sizeof(FeatvecRow));
    const int r = st.alloc();
    if (r != ORB_OK) {
        for (orb_frame_bow* B : parts) delete B;
        return r;
    }
    VocabFrameRow* vt = st.hi<VocabFrameRow>(o_vt);
    FeatvecRow* ft = st.hi<FeatvecRow>(o_ft);
    for (int f = 0; f < nframes; f++) {
        orb_frame_bow* B = parts[f];
        uint8_t* const d = B->d_base.get();
        const BowLayout& L = B->L;
        vt[f] = VocabFrameRow{frames[f]->d_desc, (int*)(d + L.o_word), (float*)(d + L.o_weight),
                              (uint32_t*)(d + L.o_tnode), frames[f]->n, 0};
        ft[f] = FeatvecRow{(const uint32_t*)(d + L.o_tnode), (const float*)(d + L.o_weight), (int*)d,
                           (uint32_t*)(d + L.o_nodes), (int*)(d + L.o_off), (int*)(d + L.o_idx),
                           (uint32_t*)(d + L.o_nodeof), frames[f]->n, vocab_empty(v) ? 1 : 0};
    }
    if ((e = launch_vocab_transform_frames(v, levelsup, st.di<VocabFrameRow>(o_vt), nframes, max_n, c->stream)) !=
        hipSuccess)
        return fail("k_vocab_transform", ORB_ERR_HIP);
    hipLaunchKernelGGL(k_frame_featvec, dim3(nframes), dim3(kFvThreads), 0, c->stream, st.di<FeatvecRow>(o_ft));
    if ((e = hipGetLastError()) != hipSuccess) return fail("k_frame_featvec", ORB_ERR_HIP);
    for (int f = 0; f < nframes; f++)
        if ((e = hipMemcpyAsync(parts[f]->h.data(), parts[f]->d_base.get(), parts[f]->L.bytes, hipMemcpyDeviceToHost,
                                c->stream)) != hipSuccess)
            return fail("orb_frame_compute_bow: copy to the host", ORB_ERR_HIP);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail("orb_frame_compute_bow: synchronise", ORB_ERR_HIP);
    for (int f = 0; f < nframes; f++) {
        orb_frame_bow* B = parts[f];
        const int* meta = B->hp<int>(0);
        B->nnodes = meta[0];
        B->nnz = meta[1];
        B->unique = true;
        if (B->nnodes < 0 || B->nnz < B->nnodes || B->nnz > frames[f]->n) {
            e = hipSuccess;
            return fail("orb_frame_compute_bow: inconsistent FeatureVector", ORB_ERR_INTERNAL);
        }
    }
    for (int f = 0; f < nframes; f++) {
        bow_attach(frames[f], parts[f]);
        parts[f] = nullptr;
    }
    return ORB_OK;
}

int orb_frame_set_featvec(orb_ctx* h, orb_frame* F, orb_featvec fv) {
    const char* const fn = "orb_frame_set_featvec";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    // (the CSR's own shape first: it needs no handle)
    if (!featvec_ok(fv, INT_MAX)) return arg_error(fn, "malformed FeatureVector CSR");
    if (!F) return arg_error(fn, "NULL frame");
    if (!featvec_ok(fv, F->n)) return arg_error(fn, "FeatureVector index outside the frame");
    const int nnz = fv.nnodes > 0 ? fv.offsets[fv.nnodes] : 0;
    for (int j = 0; j < fv.nnodes; j++)
        if (fv.node_ids[j] == kBowNoNode) return arg_error(fn, "node id 0xFFFFFFFF is reserved");
    CTX_GUARD(c);
    if (F->device != c->device) return arg_error(fn, "frame of another device");
    hipError_t e = hipSuccess;
    orb_frame_bow* B = bow_alloc(F->n, fv.nnodes, nnz, false, e);
    if (!B) return set_error("orb_frame_set_featvec: allocation", e), ORB_ERR_NOMEM;
    const BowLayout& L = B->L;
    uint8_t* const hb = B->h.data();
    int* meta = (int*)hb;
    uint32_t* nodes = (uint32_t*)(hb + L.o_nodes);
    int* off = (int*)(hb + L.o_off);
    int* idx = (int*)(hb + L.o_idx);
    uint32_t* node_of = (uint32_t*)(hb + L.o_nodeof);
    meta[0] = B->nnodes = fv.nnodes;
    meta[1] = B->nnz = nnz;
    off[0] = 0;
    for (int i = 0; i < F->n; i++) node_of[i] = kBowNoNode;
    for (int j = 0; j < fv.nnodes; j++) {
        nodes[j] = fv.node_ids[j];
        off[j + 1] = fv.offsets[j + 1];
        for (int k = fv.offsets[j]; k < fv.offsets[j + 1]; k++) {
            idx[k] = fv.indices[k];
            if (node_of[idx[k]] != kBowNoNode) B->unique = false;
            node_of[idx[k]] = fv.node_ids[j];
        }
    }
    if ((e = hipMemcpyAsync(B->d_base.get(), hb, L.bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        delete B;
        return set_error("orb_frame_set_featvec: upload", e), ORB_ERR_HIP;
    }
    bow_attach(F, B);
    return ORB_OK;
}

int orb_frame_has_bow(const orb_frame* F) { return F && F->bow ? (F->bow->triples ? 2 : 1) : 0; }

int orb_frame_bow_read(const orb_vocab* v, const orb_frame* F, int* bow_words, double* bow_values, int* nbow,
                       uint32_t* fv_nodes, int* fv_off, int* fv_idx, int* nfv) {
    const char* const fn = "orb_frame_bow_read";
    if (!F) return arg_error(fn, "NULL frame");
    if (!F->bow) return arg_error(fn, "the frame carries no BoW");
    if (!nbow || !nfv || !fv_off) return arg_error(fn, "bad arguments");
    const orb_frame_bow* B = F->bow;
    if (B->triples && (!v || (F->n > 0 && (!bow_words || !bow_values)))) return arg_error(fn, "bad arguments");
    if (B->nnz > 0 && (!fv_nodes || !fv_idx)) return arg_error(fn, "bad arguments");
    *nbow = B->triples ? vocab_bow_vector(v, F->n, B->hp<int>(B->L.o_word), B->hp<float>(B->L.o_weight), bow_words,
                                          bow_values)
                       : 0;
    const orb_featvec fv = B->featvec();
    fv_off[0] = 0;
    for (int j = 0; j < fv.nnodes; j++) {
        fv_nodes[j] = fv.node_ids[j];
        fv_off[j + 1] = fv.offsets[j + 1];
    }
    if (B->nnz > 0) std::memcpy(fv_idx, fv.indices, (size_t)B->nnz * 4);
    *nfv = fv.nnodes;
    return ORB_OK;
}

}  // extern "C"
