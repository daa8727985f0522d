// Keyframe database on gfx950 (orb_kfdb, include/orbgpu.h): the query of KeyFrameDatabase::DetectLoopCandidates /
// DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:76-309) and DBoW2's L1Scoring::score
// (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).
//
// The reference walks an inverted file (one std::list<KeyFrame*> per word) to find the keyframes that share a word
// with the query, counts the shared words, and scores those above a cut with a merge of the two BowVectors.  Here the
// live keyframes' BowVectors sit in one device pool and a query is ONE sparse intersection of the query with every
// keyframe, which yields all three results at once:
//   * the common-word count (mnLoopWords / mnRelocWords);
//   * the index, within the query, of the first common word: the reference's lKFsSharingWords is ordered by
//     (that index, the keyframe's add sequence), because the query's words are walked ascending and each word's list in
//     insertion order, so no inverted file is needed on the device: add is an append, erase a flag;
//   * the double L1Scoring::score returns, its terms added one at a time in ascending word order.
// Everything after the sharing list (the 0.8f cut, the float casts, the covisibility accumulation, the 0.75f retention)
// is order-dependent host work on a few dozen entries: orb_kfdb_candidates.
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>

#include "orbgpu_ctx.h"

struct orb_kfdb {
    int device = 0;
    // the pool: word ids ascending and values, entry after entry in add order
    orbgpu::DevBuf<int> d_words;
    orbgpu::DevBuf<double> d_vals;
    size_t pool_cap = 0, pool_used = 0, pool_dead = 0;   // in words
    // per slot (offset, length) on the device; length -1: erased.  Uploaded before a query when it has changed
    orbgpu::DevBuf<int2> d_ent;
    bool ent_dirty = false;
    std::vector<int2> ent;        // the host's copy, authoritative
    std::vector<int> slot_id;     // per slot: the id add returned
    std::vector<int> slot_of;     // per id: its slot, or -1 once erased / cleared
    std::vector<float> reloc;     // per id: mRelocScore, 0.0f until first scored (pinned)
    std::vector<char> mark;       // per slot, orb_kfdb_query: excluded
    std::vector<int> order;       // orb_kfdb_query: the sharing list's slots
    int live = 0;
};

namespace orbgpu {

constexpr int kKfdbQueryLdsWords = 4096;   // query words staged in LDS: at most 4096 * (4 + 8) B = 48 KiB per workgroup
constexpr int kKfdbThreads = 256;
constexpr int kKfdbWaves = kKfdbThreads / 64;
constexpr int kKfdbMaxBlocks = 2048;       // 8 workgroups per CU; the waves stride over the slots
constexpr size_t kKfdbInitialPool = 1024;  // words; the pool doubles from here (include/orbgpu.h states it)

// Lane l's double, l wave-uniform.
__device__ __forceinline__ double lane_double(double x, int l) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// One wave per live keyframe.  The lanes take the keyframe's words 64 at a time and look each up in the query (binary
// search: LDS, or global memory when the query is longer than the staging).  A lane with a common word holds that word's
// term fabs(vi - wi) - fabs(vi) - fabs(wi) (vi the query's value, wi the keyframe's; left to right as the reference's
// expression).  The chunk's terms are then added to the accumulator in lane order = ascending word order, ONE AT A TIME:
// the loop runs over the set bits of the ballot, wave-uniform, and every lane adds the same term read from its owner's
// register (v_readlane), so the accumulator goes through exactly the reference's sequence of partial sums.  No tree, no
// butterfly, no atomics.  The first common word of the keyframe is also the first of the query (both ascend).
template <bool LDS>
__global__ __launch_bounds__(kKfdbThreads) void k_kfdb_query(const int* __restrict__ pool_w,
                                                             const double* __restrict__ pool_v,
                                                             const int2* __restrict__ ent, int nslots,
                                                             const int* __restrict__ qw, const double* __restrict__ qv,
                                                             int nq, int* __restrict__ out_cnt,
                                                             int* __restrict__ out_first, double* __restrict__ out_score) {
    extern __shared__ double s_query[];   // LDS form: nq values, then nq words (the launch sizes it: 12 B per word)
    const double* s_v = s_query;
    const int* s_w = reinterpret_cast<const int*>(s_query + nq);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (LDS) {
        for (int i = tid; i < nq; i += kKfdbThreads) {   // nq <= kKfdbQueryLdsWords (the host picks the form)
            s_query[i] = qv[i];
            reinterpret_cast<int*>(s_query + nq)[i] = qw[i];
        }
        __syncthreads();
    }
    for (int slot = blockIdx.x * kKfdbWaves + wave; slot < nslots; slot += gridDim.x * kKfdbWaves) {
        const int2 e = ent[slot];
        const int len = e.y;
        if (len < 0) continue;   // erased (the same for the whole wave)
        const int* kw = pool_w + e.x;
        const double* kv = pool_v + e.x;
        double acc = 0.0;
        int cnt = 0, first = -1;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int i = c0 + lane;
            int idx = -1;
            double term = 0.0;
            if (i < len) {
                const int w = kw[i];
                int lo = 0, hi = nq;   // lower_bound of w in the query
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const int x = LDS ? s_w[mid] : qw[mid];
                    if (x < w)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo < nq && (LDS ? s_w[lo] : qw[lo]) == w) {
                    idx = lo;
                    const double vi = LDS ? s_v[lo] : qv[lo], wi = kv[i];
                    term = fabs(vi - wi) - fabs(vi);
                    term = term - fabs(wi);
                }
            }
            unsigned long long m = __ballot(idx >= 0);
            if (m == 0) continue;
            if (first < 0) first = __builtin_amdgcn_readlane(idx, __ffsll((long long)m) - 1);
            cnt += __popcll(m);
            while (m) {
                acc += lane_double(term, __ffsll((long long)m) - 1);   // score += ..., in word order
                m &= m - 1;
            }
        }
        if (lane == 0) {
            out_cnt[slot] = cnt;
            out_first[slot] = first;
            out_score[slot] = -acc / 2.0;   // no common word: -0.0, as the reference
        }
    }
}

namespace {

const char* bow_arg_error(int nbow, const int* words, const double* values) {
    if (nbow < 0) return "negative word count";
    if (nbow > 0 && (!words || !values)) return "NULL words / values";
    for (int i = 0; i < nbow; i++) {
        if (words[i] < 0) return "negative word id";
        if (i && words[i] <= words[i - 1]) return "words not strictly ascending";
        if (!std::isfinite(values[i])) return "value not finite";
    }
    return nullptr;
}

// L1Scoring::score (ScoringObject.cpp:23-68).  Its lower_bound skips only step over words the other vector lacks: the
// terms and their order are those of this two-pointer merge.
double l1_score(int n1, const int* w1, const double* v1, int n2, const int* w2, const double* v2) {
    double score = 0;
    for (int i = 0, j = 0; i < n1 && j < n2;) {
        if (w1[i] == w2[j]) {
            const double vi = v1[i], wi = v2[j];
            score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            i++;
            j++;
        } else if (w1[i] < w2[j]) {
            i++;
        } else {
            j++;
        }
    }
    return -score / 2.0;
}

// A pool of at least `need` words holding the live entries packed in slot order: growth (by doubling) and compaction
// are the same copy.  Runs of adjacent live entries move as one device-to-device copy.  Synchronises.
int kfdb_repack(const char* fn, Ctx* c, orb_kfdb* db, size_t need) {
    size_t cap = std::max(db->pool_cap, kKfdbInitialPool);
    while (cap < need) cap *= 2;
    if (cap > (size_t)INT_MAX) return set_error((std::string(fn) + ": pool above 2^31 words").c_str(), hipSuccess),
                                      ORB_ERR_CAPACITY;
    DevBuf<int> nw;   // the new pool: the handle's once the copy has succeeded, freed on every return before
    DevBuf<double> nv;
    hipError_t e;
    if ((e = nw.ensure(cap)) != hipSuccess || (e = nv.ensure(cap)) != hipSuccess)
        return set_error((std::string(fn) + ": pool allocation").c_str(), e), ORB_ERR_NOMEM;
    std::vector<int2> nent;
    std::vector<int> nid;
    nent.reserve(db->ent.size());
    nid.reserve(db->ent.size());
    size_t used = 0, run_src = 0, run_dst = 0, run_len = 0;
    auto flush = [&]() {
        if (run_len == 0 || e != hipSuccess) return;
        if ((e = hipMemcpyAsync(nw.get() + run_dst, db->d_words.get() + run_src, run_len * 4, hipMemcpyDeviceToDevice,
                                c->stream)) == hipSuccess)
            e = hipMemcpyAsync(nv.get() + run_dst, db->d_vals.get() + run_src, run_len * 8, hipMemcpyDeviceToDevice,
                               c->stream);
        run_len = 0;
    };
    e = hipSuccess;
    for (size_t s = 0; s < db->ent.size(); s++) {
        const int2 en = db->ent[s];
        if (en.y < 0) continue;
        if (run_len && run_src + run_len != (size_t)en.x) flush();
        if (run_len == 0) {
            run_src = (size_t)en.x;
            run_dst = used;
        }
        run_len += (size_t)en.y;
        nent.push_back(make_int2((int)used, en.y));
        nid.push_back(db->slot_id[s]);
        used += (size_t)en.y;
    }
    flush();
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return set_error((std::string(fn) + ": pool copy").c_str(), e), ORB_ERR_HIP;
    db->d_words.swap(nw);   // (the old pools leave with nw and nv)
    db->d_vals.swap(nv);
    db->pool_cap = cap;
    db->pool_used = used;
    db->pool_dead = 0;
    db->ent.swap(nent);
    db->slot_id.swap(nid);
    for (size_t s = 0; s < db->slot_id.size(); s++) db->slot_of[db->slot_id[s]] = (int)s;
    db->ent_dirty = true;
    return ORB_OK;
}

// erase only flags; the pool is packed again by the next add or query once more than half of it is dead
int kfdb_compact_if_due(const char* fn, Ctx* c, orb_kfdb* db) {
    if (db->pool_dead * 2 <= db->pool_used && db->ent.size() <= 2 * (size_t)db->live + 64) return ORB_OK;
    return kfdb_repack(fn, c, db, db->pool_used - db->pool_dead);
}

int kfdb_guard(const char* fn, Ctx* c, const orb_kfdb* db) {
    if (!c) return set_error("NULL context", hipSuccess), ORB_ERR_ARG;
    if (db->device != c->device) return arg_error(fn, "the database belongs to another device");
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return set_error("hipSetDevice", e), ORB_ERR_HIP;
    return ORB_OK;
}

}  // namespace
}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orb_kfdb_query_lds_words(void) { return kKfdbQueryLdsWords; }

int orb_bow_score(int n1, const int* w1, const double* v1, int n2, const int* w2, const double* v2, double* score) {
    const char* const fn = "orb_bow_score";
    if (!score) return arg_error(fn, "score NULL");
    if (const char* why = bow_arg_error(n1, w1, v1)) return arg_error(fn, why);
    if (const char* why = bow_arg_error(n2, w2, v2)) return arg_error(fn, why);
    *score = l1_score(n1, w1, v1, n2, w2, v2);
    return ORB_OK;
}

int orb_kfdb_create(orb_ctx* h, orb_kfdb** out) {
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!out) return arg_error("orb_kfdb_create", "out NULL");
    CTX_GUARD(c);
    orb_kfdb* db = new (std::nothrow) orb_kfdb();
    if (!db) return set_error("orb_kfdb", hipSuccess), ORB_ERR_NOMEM;
    db->device = c->device;   // the pool is allocated by the first add
    *out = db;
    return ORB_OK;
}

void orb_kfdb_destroy(orb_kfdb* db) {
    if (!db) return;
    (void)hipSetDevice(db->device);   // (freed even where this fails: hipFree takes a pointer, not the current device)
    delete db;
}

int orb_kfdb_add(orb_ctx* h, orb_kfdb* db, int nbow, const int* words, const double* values, int* id) {
    const char* const fn = "orb_kfdb_add";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!db || !id) return arg_error(fn, "NULL database or id");
    if (const char* why = bow_arg_error(nbow, words, values)) return arg_error(fn, why);
    if (db->slot_of.size() >= (size_t)INT_MAX) return arg_error(fn, "ids exhausted");
    int st = kfdb_guard(fn, c, db);
    if (st != ORB_OK) return st;
    if ((st = kfdb_compact_if_due(fn, c, db)) != ORB_OK) return st;
    if (!db->d_words || db->pool_used + (size_t)nbow > db->pool_cap)
        if ((st = kfdb_repack(fn, c, db, db->pool_used - db->pool_dead + (size_t)nbow)) != ORB_OK) return st;
    try {
        db->ent.reserve(db->ent.size() + 1);
        db->slot_id.reserve(db->slot_id.size() + 1);
        db->slot_of.reserve(db->slot_of.size() + 1);
        db->reloc.reserve(db->reloc.size() + 1);
    } catch (const std::bad_alloc&) {
        return set_error("orb_kfdb_add: host tables", hipSuccess), ORB_ERR_NOMEM;
    }
    if (nbow > 0) {
        // the caller's arrays are pageable: the copies are staged and the stream synchronised before they are released
        hipError_t e = hipMemcpyAsync(db->d_words.get() + db->pool_used, words, (size_t)nbow * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(db->d_vals.get() + db->pool_used, values, (size_t)nbow * 8, hipMemcpyHostToDevice, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return set_error("orb_kfdb_add: upload", e), ORB_ERR_HIP;
    }
    const int nid = (int)db->slot_of.size();
    db->slot_of.push_back((int)db->ent.size());
    db->reloc.push_back(0.0f);
    db->ent.push_back(make_int2((int)db->pool_used, nbow));
    db->slot_id.push_back(nid);
    db->pool_used += (size_t)nbow;
    db->live++;
    db->ent_dirty = true;
    *id = nid;
    return ORB_OK;
}

int orb_kfdb_erase(orb_kfdb* db, int id) {
    const char* const fn = "orb_kfdb_erase";
    if (!db) return arg_error(fn, "NULL database");
    if (id < 0 || (size_t)id >= db->slot_of.size() || db->slot_of[id] < 0) return arg_error(fn, "unknown or erased id");
    const int s = db->slot_of[id];
    db->pool_dead += (size_t)db->ent[s].y;
    db->ent[s].y = -1;
    db->slot_of[id] = -1;
    db->live--;
    db->ent_dirty = true;
    return ORB_OK;
}

int orb_kfdb_clear(orb_kfdb* db) {
    if (!db) return arg_error("orb_kfdb_clear", "NULL database");
    for (int s : db->slot_id) db->slot_of[s] = -1;
    db->ent.clear();
    db->slot_id.clear();
    db->pool_used = db->pool_dead = 0;
    db->live = 0;
    db->ent_dirty = true;
    return ORB_OK;
}

int orb_kfdb_size(const orb_kfdb* db) { return db ? db->live : 0; }

int orb_kfdb_query(orb_ctx* h, orb_kfdb* db, int nbow, const int* words, const double* values, int nexcl,
                   const int* excl_ids, double* excl_score, int cap, int* ids, int* common, double* score, int* n) {
    const char* const fn = "orb_kfdb_query";
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!db || !n) return arg_error(fn, "NULL database or n");
    if (const char* why = bow_arg_error(nbow, words, values)) return arg_error(fn, why);
    if (nexcl < 0 || (nexcl > 0 && !excl_ids)) return arg_error(fn, "bad exclusion list");
    if (cap < 0 || (cap > 0 && (!ids || !common || !score))) return arg_error(fn, "bad output arrays");
    for (int j = 0; j < nexcl; j++)
        if (excl_ids[j] < 0 || (size_t)excl_ids[j] >= db->slot_of.size()) return arg_error(fn, "excluded id never issued");
    int st = kfdb_guard(fn, c, db);
    if (st != ORB_OK) return st;
    if (nbow == 0 || db->live == 0) {
        // no word shared with anything: the reference's minScore loop would read -0.0 from every score()
        if (excl_score)
            for (int j = 0; j < nexcl; j++)
                if (db->slot_of[excl_ids[j]] >= 0) excl_score[j] = -0.0;
        *n = 0;
        return ORB_OK;
    }
    if ((st = kfdb_compact_if_due(fn, c, db)) != ORB_OK) return st;
    const size_t ns = db->ent.size();
    hipError_t e;
    if (ns > db->d_ent.cap()) {
        if ((e = db->d_ent.ensure(2 * ns, 256)) != hipSuccess)
            return set_error("orb_kfdb_query: entry table", e), ORB_ERR_NOMEM;
        db->ent_dirty = true;
    }
    try {
        db->mark.assign(ns, 0);
        db->order.clear();
        db->order.reserve(ns);
    } catch (const std::bad_alloc&) {
        return set_error("orb_kfdb_query: host tables", hipSuccess), ORB_ERR_NOMEM;
    }
    // [query words | query values] go up in one DMA (every workgroup reads them: not from the pinned mirror);
    // [count | first | score] per slot are stored by the kernel straight into the mirror
    Stage sg{c};
    const size_t o_qw = sg.add((size_t)nbow * 4), o_qv = sg.add((size_t)nbow * 8), o_cnt = sg.add(ns * 4),
                 o_first = sg.add(ns * 4), o_score = sg.add(ns * 8);
    if ((st = sg.alloc()) != ORB_OK) return st;
    sg.put(o_qw, words, (size_t)nbow * 4);
    sg.put(o_qv, values, (size_t)nbow * 8);
    if (db->ent_dirty) {
        if ((e = hipMemcpyAsync(db->d_ent.get(), db->ent.data(), ns * sizeof(int2), hipMemcpyHostToDevice, c->stream)) !=
            hipSuccess)
            return set_error("orb_kfdb_query: entry table upload", e), ORB_ERR_HIP;
    }
    if ((e = sg.up(o_qw, o_cnt)) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return set_error("orb_kfdb_query: upload", e), ORB_ERR_HIP;
    }
    const int blocks = (int)std::min<size_t>((ns + kKfdbWaves - 1) / kKfdbWaves, kKfdbMaxBlocks);
    if (nbow <= kKfdbQueryLdsWords)
        hipLaunchKernelGGL(k_kfdb_query<true>, dim3(blocks), dim3(kKfdbThreads), (size_t)nbow * 12, c->stream,
                           db->d_words.get(), db->d_vals.get(), db->d_ent.get(), (int)ns, sg.di<int>(o_qw),
                           sg.di<double>(o_qv), nbow, sg.h<int>(o_cnt), sg.h<int>(o_first), sg.h<double>(o_score));
    else
        hipLaunchKernelGGL(k_kfdb_query<false>, dim3(blocks), dim3(kKfdbThreads), 0, c->stream, db->d_words.get(),
                           db->d_vals.get(), db->d_ent.get(), (int)ns, sg.di<int>(o_qw), sg.di<double>(o_qv), nbow,
                           sg.h<int>(o_cnt), sg.h<int>(o_first), sg.h<double>(o_score));
    e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(c->stream);   // also when the launch failed: the uploads read db->ent
    if (e != hipSuccess) return set_error("k_kfdb_query", e), ORB_ERR_HIP;
    if (es != hipSuccess) return set_error("orb_kfdb_query: synchronise", es), ORB_ERR_HIP;
    db->ent_dirty = false;
    const int* r_cnt = sg.h<int>(o_cnt);
    const int* r_first = sg.h<int>(o_first);
    const double* r_score = sg.h<double>(o_score);
    for (int j = 0; j < nexcl; j++) {
        const int s = db->slot_of[excl_ids[j]];
        if (s >= 0) db->mark[s] = 1;
    }
    for (size_t s = 0; s < ns; s++)
        if (db->ent[s].y >= 0 && !db->mark[s] && r_cnt[s] > 0) db->order.push_back((int)s);
    *n = (int)db->order.size();
    if (*n > cap) return set_error("orb_kfdb_query: output arrays too small", hipSuccess), ORB_ERR_CAPACITY;
    // lKFsSharingWords: ascending (first common query word, add sequence); the slots are in add order
    std::stable_sort(db->order.begin(), db->order.end(), [&](int a, int b) { return r_first[a] < r_first[b]; });
    for (int i = 0; i < *n; i++) {
        const int s = db->order[i];
        ids[i] = db->slot_id[s];
        common[i] = r_cnt[s];
        score[i] = r_score[s];
    }
    if (excl_score)
        for (int j = 0; j < nexcl; j++) {
            const int s = db->slot_of[excl_ids[j]];
            if (s >= 0) excl_score[j] = r_score[s];   // an erased one: left untouched
        }
    return ORB_OK;
}

int orb_kfdb_candidates(orb_kfdb* db, int mode, float min_score, int n, const int* ids, const int* common,
                        const double* score, orb_kfdb_neighbours_fn nb, void* user, int* cand_ids, int* ncand) {
    const char* const fn = "orb_kfdb_candidates";
    if (mode != ORB_KFDB_RELOC && mode != ORB_KFDB_LOOP) return arg_error(fn, "unknown mode");
    if (!ncand || n < 0 || (n > 0 && (!ids || !common || !score || !cand_ids || !nb)))
        return arg_error(fn, "bad arguments");
    const bool loop = mode == ORB_KFDB_LOOP;
    std::unordered_map<int, int> at;        // id -> place in the sharing list
    std::unordered_map<int, float> local;   // mRelocScore of a call without a handle
    int maxCommonWords = 0;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || (db && (size_t)ids[i] >= db->slot_of.size())) return arg_error(fn, "id never issued");
        if (common[i] < 1) return arg_error(fn, "common-word count below 1");
        if (!at.emplace(ids[i], i).second) return arg_error(fn, "id listed twice");
        if (common[i] > maxCommonWords) maxCommonWords = common[i];
    }
    *ncand = 0;
    if (n == 0) return ORB_OK;   // if(lKFsSharingWords.empty()) return (:107, :224)
    const int minCommonWords = maxCommonWords * 0.8f;   // :120, :235: int -> float, float product, truncation
    auto reloc_of = [&](int id) -> float& { return db ? db->reloc[id] : local[id]; };   // (local: 0.0f when new)
    // Compute similarity score (:125-139, :242-253)
    std::vector<float> si(n, 0.0f);
    std::vector<int> lScoreAndMatch;
    for (int i = 0; i < n; i++) {
        if (common[i] <= minCommonWords) continue;
        si[i] = (float)score[i];
        if (loop) {
            if (si[i] >= min_score) lScoreAndMatch.push_back(i);
        } else {
            reloc_of(ids[i]) = si[i];
            lScoreAndMatch.push_back(i);
        }
    }
    if (lScoreAndMatch.empty()) return ORB_OK;
    // accumulate score by covisibility (:148-173, :262-287)
    std::vector<std::pair<float, int>> lAccScoreAndMatch;
    float bestAccScore = loop ? min_score : 0;
    int neigh[10];
    for (int i : lScoreAndMatch) {
        const int nn = nb(user, ids[i], neigh, 10);   // GetBestCovisibilityKeyFrames(10)
        if (nn < 0 || nn > 10) return arg_error(fn, "the neighbour callback returned a count outside [0, 10]");
        float bestScore = si[i], accScore = si[i];
        int best = ids[i];
        for (int k = 0; k < nn; k++) {
            const auto it = at.find(neigh[k]);
            if (it == at.end()) continue;   // mnLoopQuery / mnRelocQuery is not this query
            float s;
            if (loop) {
                if (common[it->second] <= minCommonWords) continue;
                s = si[it->second];   // mLoopScore of this query, also below min_score
            } else {
                s = reloc_of(neigh[k]);   // below the cut: what the last query that scored it left
            }
            accScore += s;
            if (s > bestScore) {
                best = neigh[k];
                bestScore = s;
            }
        }
        lAccScoreAndMatch.emplace_back(accScore, best);
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    // Return all those keyframes with a score higher than 0.75*bestScore (:176-193, :290-306)
    const float minScoreToRetain = 0.75f * bestAccScore;
    int m = 0;
    for (const auto& a : lAccScoreAndMatch) {
        if (!(a.first > minScoreToRetain)) continue;
        bool seen = false;
        for (int k = 0; k < m && !seen; k++) seen = cand_ids[k] == a.second;
        if (!seen) cand_ids[m++] = a.second;
    }
    *ncand = m;
    return ORB_OK;
}

}  // extern "C"
