// Single-thread CPU baseline of tools/kfdb_latency.py: the keyframe-database query as the reference structures it
// (KeyFrameDatabase::DetectRelocalizationCandidates up to the scores): one std::list of keyframes per word, the query's
// words walked in order with per-keyframe marks, the 0.8f cut, and DBoW2's L1 score (a merge of two std::map
// BowVectors with lower_bound skips) for the keyframes above the cut.  Written for this project; no SLAM types.
//
//   kfdb_cpu_query <vectors.bin> <repetitions>
// vectors.bin: int32 count, then per vector int32 n, int32 words[n], double values[n]; the last vector is the query,
// the others are added in order.  Prints one JSON line: median / min microseconds per query, listed and scored counts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <list>
#include <map>
#include <unordered_map>
#include <vector>

typedef std::map<unsigned, double> BowVector;

struct KF {
    BowVector bow;
    long query = -1000;   // the repetition that listed it last
    int words = 0;
    float score = 0;
};

static double l1_score(const BowVector& v1, const BowVector& v2) {
    BowVector::const_iterator a = v1.begin(), b = v2.begin();
    double score = 0;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) {
            score += fabs(a->second - b->second) - fabs(a->second) - fabs(b->second);
            ++a;
            ++b;
        } else if (a->first < b->first) {
            a = v1.lower_bound(b->first);
        } else {
            b = v2.lower_bound(a->first);
        }
    }
    return -score / 2.0;
}

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s vectors.bin repetitions\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    const int reps = atoi(argv[2]);
    int32_t count = 0;
    if (!f || reps < 1 || fread(&count, 4, 1, f) != 1 || count < 1) return fprintf(stderr, "bad input\n"), 2;
    std::vector<KF> kfs(count);
    for (int k = 0; k < count; k++) {
        int32_t n = 0;
        if (fread(&n, 4, 1, f) != 1 || n < 0) return fprintf(stderr, "bad input\n"), 2;
        std::vector<int32_t> w(n);
        std::vector<double> v(n);
        if (n && (fread(w.data(), 4, n, f) != (size_t)n || fread(v.data(), 8, n, f) != (size_t)n))
            return fprintf(stderr, "bad input\n"), 2;
        for (int i = 0; i < n; i++) kfs[k].bow[(unsigned)w[i]] = v[i];
    }
    fclose(f);
    const BowVector query = kfs.back().bow;
    kfs.pop_back();
    std::unordered_map<unsigned, std::list<KF*> > inverted;   // (the reference: a vector sized by the vocabulary)
    for (KF& k : kfs)
        for (const auto& e : k.bow) inverted[e.first].push_back(&k);

    std::vector<double> us;
    size_t listed = 0, scored = 0;
    double sink = 0;
    for (int r = -3; r < reps; r++) {   // three warm-up queries
        const auto t0 = std::chrono::steady_clock::now();
        std::list<KF*> sharing;
        for (const auto& e : query) {
            const auto it = inverted.find(e.first);
            if (it == inverted.end()) continue;
            for (KF* k : it->second) {
                if (k->query != r) {
                    k->words = 0;
                    k->query = r;
                    sharing.push_back(k);
                }
                k->words++;
            }
        }
        int maxCommonWords = 0;
        for (KF* k : sharing) maxCommonWords = std::max(maxCommonWords, k->words);
        const int minCommonWords = maxCommonWords * 0.8f;
        size_t ns = 0;
        for (KF* k : sharing)
            if (k->words > minCommonWords) {
                k->score = (float)l1_score(query, k->bow);
                sink += k->score;
                ns++;
            }
        const auto t1 = std::chrono::steady_clock::now();
        if (r >= 0) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        listed = sharing.size();
        scored = ns;
    }
    std::sort(us.begin(), us.end());
    printf("{\"cpu_query_us_median\": %.2f, \"cpu_query_us_min\": %.2f, \"listed\": %zu, \"scored\": %zu, \"reps\": %d, "
           "\"checksum\": %.6f}\n",
           us[us.size() / 2], us[0], listed, scored, reps, sink);
    return 0;
}
