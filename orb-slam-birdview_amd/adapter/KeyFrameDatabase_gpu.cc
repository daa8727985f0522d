/*
 * KeyFrameDatabase_gpu.cc — ORB_SLAM2::KeyFrameDatabase with the reference's exact member signatures
 * (include/KeyFrameDatabase.h:42-70 of donglinb/ORB-SLAM-BIRDVIEW), computed by liborbgpu.
 *
 * This file is compiled INSIDE the reference's libORB_SLAM2 IN PLACE OF src/KeyFrameDatabase.cc:
 *
 *   KeyFrameDatabase(const ORBVocabulary&)                              KeyFrameDatabase.cc:33-37
 *   void add(KeyFrame*) / erase(KeyFrame*) / clear()                    :40-73
 *   vector<KeyFrame*> DetectLoopCandidates(KeyFrame*, float minScore)   :76-197
 *   vector<KeyFrame*> DetectRelocalizationCandidates(Frame*)            :199-309
 *
 * The header is the reference's own and stays unchanged, so what the GPU form needs per database (its liborbgpu
 * context, the orb_kfdb handle and the KeyFrame* <-> id map) lives in a table keyed by the object's address, created by
 * the constructor.  The reference's class has no destructor: an entry lives as long as the process (the reference owns
 * one database for the life of its System).  mvInvertedFile stays empty.
 *
 * The BowVectors of the keyframes sit on the GPU (add uploads mBowVec once); a Detect* call is one kernel launch that
 * intersects the query with every keyframe (orb_kfdb_query) followed by the reference's order-dependent tail on the
 * host (orb_kfdb_candidates), which calls KeyFrame::GetBestCovisibilityKeyFrames(10) for exactly the keyframes the
 * reference calls it for, in the same order.  Returned vectors equal the reference's, given that mRelocScore starts at
 * 0.0f (the reference leaves it uninitialised).  The members KeyFrame::mnLoopQuery / mnLoopWords / mLoopScore /
 * mnRelocQuery / mnRelocWords / mRelocScore are not written (nothing else in the reference reads them).
 *
 * Thread safety: every member locks mMutex for its whole duration (the reference locks it around the inverted-file
 * walks only): the handle and its context serve one thread at a time.  GetBestCovisibilityKeyFrames is therefore called
 * with mMutex held; KeyFrame takes its own mutexes inside and never calls into the database while holding them
 * (KeyFrame::SetBadFlag calls erase after its locked blocks, KeyFrame.cc:468-560), so the lock order is one-way.
 * A GPU failure throws std::runtime_error (the reference has no error path; there is no CPU fallback).
 */
#include "KeyFrameDatabase.h"

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/orbgpu.h"

namespace ORB_SLAM2 {

namespace orbgpu_kfdb {

void check(int st, const char* what) {
    if (st != ORB_OK) throw std::runtime_error(std::string("liborbgpu ") + what + ": " + orb_last_error());
}

struct State {
    orb_ctx* ctx = nullptr;
    orb_kfdb* db = nullptr;
    std::map<KeyFrame*, int> id_of;   // live keyframes
    std::vector<KeyFrame*> kf_of;     // per id (also erased ones: they are never looked up again)
    ~State() {
        if (db) orb_kfdb_destroy(db);
        if (ctx) orb_destroy(ctx);
    }
};

std::mutex table_mutex;
std::map<const KeyFrameDatabase*, std::unique_ptr<State> > table;

State& state_of(const KeyFrameDatabase* self, bool fresh = false) {
    std::unique_lock<std::mutex> lock(table_mutex);
    std::unique_ptr<State>& s = table[self];
    if (fresh) s.reset();   // a new object at the address of a destroyed one
    if (!s) {
        s.reset(new State());
        const char* e = getenv("ORBGPU_DEVICE");
        orb_params p;
        memset(&p, 0, sizeof p);
        p.nfeatures = 1000;   // extraction parameters are unused by the database entry points
        p.scaleFactor = 1.2f;
        p.nlevels = 8;
        p.iniThFAST = 20;
        p.minThFAST = 7;
        p.device = e ? atoi(e) : 0;
        int st = ORB_OK;
        s->ctx = orb_create(&p, &st);
        if (!s->ctx) check(st, "orb_create");
        check(orb_kfdb_create(s->ctx, &s->db), "orb_kfdb_create");
    }
    return *s;
}

// DBoW2::BowVector (a std::map<WordId, WordValue>: ascending words) as the C-ABI's two arrays
void flatten(const DBoW2::BowVector& v, std::vector<int>& w, std::vector<double>& x) {
    w.clear();
    x.clear();
    w.reserve(v.size());
    x.reserve(v.size());
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
        if (it->first > (unsigned)INT_MAX) throw std::runtime_error("liborbgpu: word id above 2^31 - 1");
        w.push_back((int)it->first);
        x.push_back(it->second);
    }
}

struct Neighbours {
    State* s;
};

// orb_kfdb_neighbours_fn: KeyFrame::GetBestCovisibilityKeyFrames(cap) of keyframe `id`, as ids.  A neighbour the
// database does not hold cannot be in the sharing list: it is passed as an id no list contains (INT_MAX).
int neighbours(void* user, int id, int* out, int cap) {
    State& s = *static_cast<Neighbours*>(user)->s;
    const std::vector<KeyFrame*> v = s.kf_of[id]->GetBestCovisibilityKeyFrames(cap);
    int n = 0;
    for (size_t i = 0; i < v.size() && n < cap; i++) {
        const std::map<KeyFrame*, int>::const_iterator it = s.id_of.find(v[i]);
        out[n++] = it == s.id_of.end() ? INT_MAX : it->second;
    }
    return n;
}

std::vector<KeyFrame*> detect(State& s, int mode, const DBoW2::BowVector& bow, const std::vector<int>& excl,
                              float minScore) {
    std::vector<int> w;
    std::vector<double> x;
    flatten(bow, w, x);
    const int cap = orb_kfdb_size(s.db);
    std::vector<int> ids(cap + 1), common(cap + 1), cand(cap + 1);
    std::vector<double> score(cap + 1);
    int n = 0, nc = 0;
    check(orb_kfdb_query(s.ctx, s.db, (int)w.size(), w.data(), x.data(), (int)excl.size(), excl.data(), nullptr, cap,
                         ids.data(), common.data(), score.data(), &n),
          "orb_kfdb_query");
    Neighbours nb{&s};
    check(orb_kfdb_candidates(s.db, mode, minScore, n, ids.data(), common.data(), score.data(), neighbours, &nb,
                              cand.data(), &nc),
          "orb_kfdb_candidates");
    std::vector<KeyFrame*> out;
    out.reserve(nc);
    for (int i = 0; i < nc; i++) out.push_back(s.kf_of[cand[i]]);
    return out;
}

}  // namespace orbgpu_kfdb

using namespace orbgpu_kfdb;

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc) : mpVoc(&voc) { state_of(this, true); }

void KeyFrameDatabase::add(KeyFrame* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    State& s = state_of(this);
    if (s.id_of.count(pKF)) return;   // (the reference would list it twice; its callers add a keyframe once)
    std::vector<int> w;
    std::vector<double> x;
    flatten(pKF->mBowVec, w, x);
    int id = -1;
    check(orb_kfdb_add(s.ctx, s.db, (int)w.size(), w.data(), x.data(), &id), "orb_kfdb_add");
    if ((size_t)id >= s.kf_of.size()) s.kf_of.resize((size_t)id + 1, nullptr);
    s.kf_of[id] = pKF;
    s.id_of[pKF] = id;
}

void KeyFrameDatabase::erase(KeyFrame* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    State& s = state_of(this);
    const std::map<KeyFrame*, int>::iterator it = s.id_of.find(pKF);
    if (it == s.id_of.end()) return;   // not in the inverted file: the reference's loops find nothing to remove
    check(orb_kfdb_erase(s.db, it->second), "orb_kfdb_erase");
    s.id_of.erase(it);
}

void KeyFrameDatabase::clear() {
    std::unique_lock<std::mutex> lock(mMutex);
    State& s = state_of(this);
    check(orb_kfdb_clear(s.db), "orb_kfdb_clear");
    s.id_of.clear();
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore) {
    const std::set<KeyFrame*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();   // (:78, before the lock)
    std::unique_lock<std::mutex> lock(mMutex);
    State& s = state_of(this);
    std::vector<int> excl;
    for (std::set<KeyFrame*>::const_iterator it = spConnectedKeyFrames.begin(); it != spConnectedKeyFrames.end(); ++it) {
        const std::map<KeyFrame*, int>::const_iterator f = s.id_of.find(*it);
        if (f != s.id_of.end()) excl.push_back(f->second);
    }
    return detect(s, ORB_KFDB_LOOP, pKF->mBowVec, excl, minScore);
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F) {
    std::unique_lock<std::mutex> lock(mMutex);
    return detect(state_of(this), ORB_KFDB_RELOC, F->mBowVec, std::vector<int>(), 0.f);
}

}  // namespace ORB_SLAM2
