// liborbgpu context (the object behind the opaque orb_ctx*).
#pragma once
#include <algorithm>
#include <array>
#include <cstring>
#include <string>
#include <vector>

#include "buf.h"
#include "orbgpu_internal.h"

namespace orbgpu {

void set_error(const char* what, hipError_t e);

// A refused argument: the message "<fn>: <why>" for orb_last_error(), and the status.
inline int arg_error(const char* fn, const std::string& why) {
    return set_error((std::string(fn) + ": " + why).c_str(), hipSuccess), ORB_ERR_ARG;
}

// An entry point's first use of its context: NULL is refused, the context's device made current.
#define CTX_GUARD(ctx)                                                                    \
    if (!(ctx)) return orbgpu::set_error("NULL context", hipSuccess), ORB_ERR_ARG;        \
    {                                                                                     \
        hipError_t _e = hipSetDevice((ctx)->device);                                      \
        if (_e != hipSuccess) return orbgpu::set_error("hipSetDevice", _e), ORB_ERR_HIP;  \
    }

// Buf's memory policies: device memory, pinned host memory with the default flags, and pinned host memory the kernels
// store into directly (mapped + coherent: the host reads it after a stream synchronisation, with no D2H copy)
struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
};
struct MappedMem {
    static hipError_t alloc(void** p, size_t bytes) {
        return hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
    }
    static void free(void* p) { (void)hipHostFree(p); }
};
template <class T>
using DevBuf = Buf<T, DeviceMem>;
template <class T>
using PinBuf = Buf<T, PinnedMem>;
template <class T>
using MapBuf = Buf<T, MappedMem>;

struct ProfPair {
    int id;
    hipEvent_t b, e;
};

struct Ctx {
    orb_params p{};
    int device = 0;
    int num_cu = 256;
    bool fast_stamps = false;     // ORBGPU_FAST_STAMPS=1: the kernels record phase timestamps (diagnostic)
    bool stereo_stage = false;    // ORBGPU_STEREO_STAGE=1: stereo stages the right side as for a peer GPU (test)
    DevBuf<unsigned long long> d_stamps;
    hipStream_t stream = nullptr;
    // the host path's second stream and fork / join events (Ctx::run_extract latency mode; ORBGPU_FORK=1: on.  Off by
    // default: 0.1154-0.1198 ms per C3 frame forked against 0.1074 ms in one stream, profiles/r04/v3_host_path.txt)
    bool fork = false;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;

    // ORBextractor tables (ORBextractor.cc:410-470)
    float scale[ORBGPU_MAX_LEVELS]{}, inv_scale[ORBGPU_MAX_LEVELS]{}, sigma2[ORBGPU_MAX_LEVELS]{},
        inv_sigma2[ORBGPU_MAX_LEVELS]{};
    int n_per_level[ORBGPU_MAX_LEVELS]{};
    int umax[16]{};
    bool umax_ok = false;
    int gk[8]{};

    // geometry of the current image size
    bool have_geom = false;
    Geom geom{};
    int rcoef_off[ORBGPU_MAX_LEVELS]{};
    DevBuf<Geom> d_geom;
    DevBuf<ResizeCoef> d_rcoef;
    DevBuf<ChainJob> d_chain;   // the one-launch pyramid's jobs (small batches)
    ChainPlan chain{};
    std::vector<ChainJob> chain_jobs_host;   // (the dataflow launch's chain tasks index them)
    DevBuf<ChainJob> d_chain2;  // the small-batch plan (levels past kSmallChainBase in one launch)
    ChainPlan chain_small{};
    DevBuf<CellDesc> d_cells;

    // extractor work buffers
    DevBuf<uint8_t> d_pyr;
    DevBuf<uint32_t> d_cands;
    DevBuf<uint32_t> d_candFirst;
    DevBuf<uint32_t> d_keys;
    DevBuf<uint16_t> d_knode;
    DevBuf<uint32_t> d_lvlKps;
    DevBuf<int> d_lvlCount;
    DevBuf<int> d_err;

    // host-image path (extract_host)
    DevBuf<uint8_t> d_in;
    // streamed upload (k_upload_stream; off by default, ORBGPU_UPLOAD=1 turns it on; off = the pageable
    // hipMemcpy2DAsync): the image's pinned host-coherent staging copy and the per-band flags the host raises (call
    // sequence numbers)
    bool upload_stream = false;
    MapBuf<uint8_t> h_img;
    MapBuf<uint32_t> h_flags;
    uint32_t upload_seq = 0;
    // extract_host's outputs [count | flag | pad | keypoints | descriptors]: host-coherent pinned memory the
    // kernels write directly (no download)
    MapBuf<uint8_t> h_pinned;

    // orb_search_for_triangulation's host lists, kept across calls (capacity reused: a call is ~30 us, and its
    // dozens of small allocations were a measurable part of it)
    std::vector<int> tri_item_q, tri_train_of, tri_best, tri_match, tri_ranges;
    std::vector<int> tri_hist[30];
    // orb_hamming_top2_frames_device: the pair list on the device (re-uploaded only when it changes), the list it
    // holds, and two pinned staging slots used in turn
    DevBuf<int2> d_pairs;
    std::vector<int> pairs_last;
    PinBuf<int2> h_pairs[2];
    hipEvent_t pairs_ev[2] = {nullptr, nullptr};
    int pairs_slot = 0;
    // matcher scratch arena (bytes)
    DevBuf<uint8_t> d_scratch;
    // pinned mirror of the matcher arena: a call's inputs are packed here at the device offsets and go up
    // in one DMA, its outputs come back in one (matcher.hip Stage)
    MapBuf<uint8_t> h_mstage;
    // the right extractor's frame + pyramid when it runs on another GPU (orb_compute_stereo_matches)
    DevBuf<uint8_t> d_peer;

    // last batch (for the mvImagePyramid view and debug reads)
    const uint8_t* last_frames = nullptr;
    long long last_frame_pitch = 0;
    int last_row_stride = 0;
    int last_nframes = 0;
    const orb_keypoint* last_kps = nullptr;   // outputs of the last batch (stereo matching reads them)
    const uint8_t* last_desc = nullptr;
    const int* last_counts = nullptr;
    int last_kp_cap = 0;
    unsigned level_cache_valid = 0;
    std::vector<uint8_t> level_host[ORBGPU_MAX_LEVELS];

    // profiling
    bool prof_on = false;
    // Replay of the per-batch launch sequence as a HIP graph (ORBGPU_GRAPH=0 disables): captured on the
    // first batch with a given set of buffers / arguments and re-instantiated when any of them changes
    bool use_graph = true;
    unsigned geom_serial = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    std::array<uintptr_t, 24> gkey{};
    hipEvent_t prof_open[ORB_K_COUNT]{};
    std::vector<ProfPair> prof_pairs;

    // the small-batch dataflow launch (k_extract_flow): batches of at most flow_max_frames frames take it
    // (ORBGPU_FLOW=1; 0, the default, keeps the per-kernel launches); its task list per (geometry, frame count), the
    // counters it waits on
    int flow_max_frames = 0;
    int flow_blocks = 0;            // workgroups per launch (ORBGPU_FLOW_BLOCKS; 0: the default, kFlowDefaultBlocks)
    DevBuf<FlowTask> d_flow;
    DevBuf<int> d_flow_ctr;
    FlowPlan flow{};
    ChainPlan flow_chain_plan{};
    DevBuf<FlowArgs> d_flow_args;  // the last uploaded arguments (h_flow_args mirrors them)
    FlowArgs h_flow_args{};
    bool flow_args_valid = false;
    bool flow_stamps = false;       // ORBGPU_FLOW_STAMPS=1: per-task timestamps (orb_debug_fast_stamps returns them)
    DevBuf<unsigned long long> d_flow_stamps;
    unsigned flow_serial = 0;       // geom_serial the plan was built for
    bool flow_ok = false;           // flow holds a plan for (flow_serial, flow.nframes)

    // MapPoint::PredictScale's level thresholds (point_project.h), found once per (log_scale_factor, nlevels)
    struct LevelThresholds {
        float lsf;
        int nlevels;
        float T[ORBGPU_MAX_LEVELS];
    };
    std::vector<LevelThresholds> level_thr;

    // k_undistort_fisheye's guard band (undistort.hip): 0 = the default, else orb_debug_undistort_guard's override
    double undistort_guard = 0.0;

    int ensure_geometry(int W, int H);
    int ensure_flow(int nframes);
    int ensure_frames(int nframes);
    ExtractBuffers buffers() const;
    // err: the overflow flag the kernels raise (default d_err); err_host: a host-coherent word k_describe
    // copies it to (orb_extract, whose kernels write their outputs straight into pinned memory)
    int run_extract(const uint8_t* d_frames, int nframes, long long frame_pitch, int row_stride, orb_keypoint* d_kps,
                    uint8_t* d_desc, int* d_counts, int kp_cap, int* err = nullptr, bool latency = false,
                    int* err_host = nullptr);
    static void marker(void* user, int id, int begin, hipStream_t s);
};

// The context's device scratch arena (Ctx::d_scratch): reserve the total first, then take() pieces.
struct Arena {
    Ctx* c;
    size_t off = 0;
    static size_t align(size_t x) { return (x + 255) & ~(size_t)255; }
    hipError_t reserve(size_t bytes) { return c->d_scratch.ensure(bytes); }
    template <class T>
    T* take(size_t n) {
        off = align(off);
        T* p = (T*)(c->d_scratch.get() + off);
        off += std::max<size_t>(n, 1) * sizeof(T);
        return p;
    }
};

inline size_t pitch64(size_t row_bytes) { return (std::max<size_t>(row_bytes, 1) + 63) & ~(size_t)63; }

// A host image of `rows` rows of row_bytes bytes into the arena, rows padded to 64 bytes (pitch64: the dword paths of
// k_to_gray and k_remap then hold for every row), by hipMemcpy2DAsync on the context's stream.  The arena is reserved
// here, for the image and `extra` bytes the caller takes after it; an empty image uploads nothing.  ORB_OK and d_img,
// or the status to return, with what_alloc / what_copy as the error text.
int upload_to_arena(Arena& a, const uint8_t* img, size_t row_bytes, int rows, size_t stride, size_t extra,
                    const char* what_alloc, const char* what_copy, uint8_t** d_img);

// The image a host-image entry point was given: w x h pixels, rows `stride` bytes apart.  color >= 0: a colour image
// with that ORB_COLOR_* code, converted to gray on the device; rect: a raw gray image to rectify on the device, the
// extracted image then has the maps' size; prep: the fisheye camera's frame (color is then its front-image code,
// ORB_PREP_GRAY included), masked, cropped, halved and converted on the device, the extracted image then has
// orb_prep_size's size.  None of them: the gray image itself.
struct HostImage {
    const uint8_t* data;
    int w, h;
    size_t stride;
    int color = -1;
    const orb_rectify* rect = nullptr;
    const orb_prep* prep = nullptr;
};

// orb_extract, orb_extract_color, orb_extract_rectified and orb_extract_fisheye behind their argument checks (orbgpu_abi.hip): the image
// staged into Ctx::d_in as a gray frame, the single-frame chain, one synchronisation, the outputs copied out.  The
// chain sees the same frame whatever the form, so orb_get_level(ctx, 0) is the gray / rectified image.
int extract_host(Ctx* c, const HostImage& im, orb_keypoint* kps, int cap, int* n, uint8_t* desc);

// A host call's device arena and its pinned host mirror (Ctx::h_mstage): regions are laid out once
// with add(), inputs are written into the mirror at the device offsets, one DMA takes the input span up
// (or the kernels read the mirror itself, zc = 1), and the kernels store their outputs straight into the mirror
// (host-coherent), so nothing is downloaded.  Regions added after end_mirror() are device-only working space:
// the pinned mirror is not sized for them.
struct Stage {
    Ctx* c;
    size_t off = 0;
    size_t mirror_end = 0;   // 0: every region has a host mirror
    // the call's input mode.  r04 per call (profiles/r04/v3_matcher_zc.txt): the single-kernel calls with small
    // inputs (SearchForTriangulation, ComputeBoW) gain from reading the pinned mirror (zc = 1: no DMA before the
    // kernel); the searches whose kernels re-read their inputs many times (the BoW searches, the window search:
    // every candidate's descriptor; stereo) lose, so they keep the DMA (zc = 0)
    int zc = 0;
    size_t add(size_t bytes) {
        off = Arena::align(off);
        const size_t o = off;
        off += std::max<size_t>(bytes, 1);
        return o;
    }
    void end_mirror() { mirror_end = Arena::align(off); }
    int alloc() {
        const size_t need = Arena::align(off) + 4096;
        Arena a{c};
        hipError_t e = a.reserve(need);
        if (e != hipSuccess) return set_error("matcher scratch", e), ORB_ERR_NOMEM;
        const size_t hneed = (mirror_end ? mirror_end : Arena::align(off)) + 4096;
        // (mapped + coherent: the matcher kernels store their results straight into this mirror)
        if ((e = c->h_mstage.ensure(hneed, 1 << 20)) != hipSuccess)
            return set_error("matcher pinned staging", e), ORB_ERR_NOMEM;
        return ORB_OK;
    }
    template <class T>
    T* h(size_t o) const { return reinterpret_cast<T*>(c->h_mstage.get() + o); }   // outputs (host view)
    template <class T>
    T* d(size_t o) const { return reinterpret_cast<T*>(c->d_scratch.get() + o); }
    template <class T>
    T* hi(size_t o) const { return reinterpret_cast<T*>(c->h_mstage.get() + o); }   // inputs, written by the host
    template <class T>
    T* di(size_t o) const {   // inputs, as the kernels read them
        return zc ? reinterpret_cast<T*>(c->h_mstage.get() + o) : d<T>(o);
    }
    void put(size_t o, const void* src, size_t bytes) const {   // an input region's content (nothing: src may be NULL)
        if (bytes) std::memcpy(hi<uint8_t>(o), src, bytes);
    }
    hipError_t up(size_t from, size_t to) const {
        if (zc) return hipSuccess;   // the kernels read the pinned mirror itself
        return to > from ? hipMemcpyAsync(d<uint8_t>(from), h<uint8_t>(from), to - from, hipMemcpyHostToDevice, c->stream)
                         : hipSuccess;
    }
    hipError_t down(size_t from, size_t to) const {
        return to > from ? hipMemcpyAsync(h<uint8_t>(from), d<uint8_t>(from), to - from, hipMemcpyDeviceToHost, c->stream)
                         : hipSuccess;
    }
};

}  // namespace orbgpu

// A resident frame's BoW part (frame_bow.hip): an allocation of its own, laid out by bow_layout() as
// [meta | fv_nodes | fv_off | fv_idx | node_of | word | weight | tnode], each region 256-byte aligned:
//   meta     2 ints: nnodes, nnz (written by k_frame_featvec; the host copy is authoritative after the attach)
//   fv_*     the FeatureVector as CSR: node ids strictly ascending, nnodes + 1 offsets, a node's features ascending
//            (n, n + 1 and n slots, or as many as a given CSR holds)
//   node_of  per feature its FeatureVector node, kBowNoNode outside the FeatureVector
//   word / weight / tnode   k_vocab_transform's per-feature triples (orb_frame_compute_bow only)
// `h` is the host copy of the whole allocation, filled by the attach's one synchronisation (orb_frame_compute_bow) or
// built on the host and uploaded (orb_frame_set_featvec); the replays and orb_frame_bow_read use it.
namespace orbgpu {
constexpr uint32_t kBowNoNode = 0xFFFFFFFFu;
struct BowLayout {
    size_t o_nodes, o_off, o_idx, o_nodeof, o_word, o_weight, o_tnode, bytes;
};
// n features, room for ncap nodes and icap indices (n of each for a FeatureVector transform() builds; a given one may
// hold empty nodes and list a feature twice)
inline BowLayout bow_layout(int n, int ncap, int icap, bool triples) {
    const auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t nn = (size_t)n;
    BowLayout L{};
    L.o_nodes = 256;
    L.o_off = al(L.o_nodes + (size_t)ncap * 4);
    L.o_idx = al(L.o_off + ((size_t)ncap + 1) * 4);
    L.o_nodeof = al(L.o_idx + (size_t)icap * 4);
    L.o_word = al(L.o_nodeof + nn * 4);
    L.o_weight = triples ? al(L.o_word + nn * 4) : L.o_word;
    L.o_tnode = triples ? al(L.o_weight + nn * 4) : L.o_word;
    L.bytes = triples ? al(L.o_tnode + nn * 4) : L.o_word;
    return L;
}
}  // namespace orbgpu
struct orb_frame_bow {
    orbgpu::DevBuf<uint8_t> d_base;
    std::vector<uint8_t> h;
    orbgpu::BowLayout L{};
    bool triples = false;
    bool unique = true;   // no feature is listed twice (a FeatureVector built by transform(); a given one may)
    int nnodes = 0, nnz = 0;
    template <class T>
    const T* d(size_t o) const { return reinterpret_cast<const T*>(d_base.get() + o); }
    template <class T>
    const T* hp(size_t o) const { return reinterpret_cast<const T*>(h.data() + o); }
    orb_featvec featvec() const {   // the host CSR copy
        return orb_featvec{nnodes, hp<uint32_t>(L.o_nodes), hp<int>(L.o_off), hp<int>(L.o_idx)};
    }
};

// A device-resident Frame / KeyFrame (the object behind the opaque orb_frame*, frame.hip): the train side of the grid
// searches, uploaded once.  One device allocation holds [desc | kps | uright | cell_off | cell_idx], each region
// 256-byte aligned; cell_off / cell_idx are the Frame grid k_frame_grid built from the keypoints.  The host keeps the
// keypoints: the searches' replays read their octave and angle.
struct orb_frame {
    int device = 0;
    int n = 0;
    bool has_ur = false;
    float min_x = 0, min_y = 0, inv_w = 0, inv_h = 0;
    orbgpu::DevBuf<uint8_t> d_base;
    const uint8_t* d_desc = nullptr;
    const orb_keypoint* d_kps = nullptr;
    const float* d_ur = nullptr;   // NULL: created without uright
    const int* d_coff = nullptr;   // kFrameGridCells + 1
    const int* d_cidx = nullptr;   // n slots (cell_off[kFrameGridCells] of them used)
    std::vector<orb_keypoint> kps;
    int oct_min = 0, oct_max = -1;   // the octaves of kps, found once by the creator (n > 0)
    // the optional BoW part, owned (orb_frame_compute_bow / orb_frame_set_featvec attach it; again: replace it)
    orb_frame_bow* bow = nullptr;
    orb_frame() = default;
    orb_frame(const orb_frame&) = delete;
    orb_frame& operator=(const orb_frame&) = delete;
    ~orb_frame() { delete bow; }
};

namespace orbgpu {

// A FeatureVector CSR the walks can trust (matcher.hip): offsets start at 0 and never decrease, every feature index
// lies in [0, n), node ids ascend strictly.  O(nnodes + nnz).
bool featvec_ok(const orb_featvec& v, int n);

// vocab.hip, for frame_bow.hip (orb_vocab is defined there).  One k_vocab_transform launch over nframes resident
// frames: row f of d_tab names frame f's descriptors, count and the three output arrays; max_n the largest count.
struct VocabFrameRow {
    const uint8_t* desc;
    int* word;
    float* weight;
    uint32_t* node;
    int n;
    int pad;
};
hipError_t launch_vocab_transform_frames(const orb_vocab* v, int levelsup, const VocabFrameRow* d_tab, int nframes,
                                         int max_n, hipStream_t stream);
int vocab_device(const orb_vocab* v);
bool vocab_empty(const orb_vocab* v);   // no words: transform() returns empty vectors
// orb_vocab_bow's BowVector half (words ascending, values in double, summed in feature order, normalised): the count
int vocab_bow_vector(const orb_vocab* v, int n, const int* word_id, const float* weight, int* bow_words,
                     double* bow_values);

// The one place the handle is laid out (frame.hip): F for n keypoints over grid g, its allocation made, the five device
// pointers set (d_ur only with has_ur), the host keypoint copy sized but not filled.  nullptr, or the step that failed
// for the caller's fail(what, ORB_ERR_NOMEM), with its HIP error in e; F is then nullptr and nothing is left allocated.
const char* frame_alloc(Ctx* c, int n, bool has_ur, const ProjGrid& g, orb_frame*& F, hipError_t& e);

// oct_min / oct_max from the host keypoints, once they hold the frame's final records
void frame_octaves(orb_frame* F);

}  // namespace orbgpu
