// Drives adapter/KeyFrameDatabase_gpu.cc (the reference's member signatures) over the models in slam_api/ with the
// script tests/test_gpu_kfdb_adapter.py writes (tests/kfdb_cases.py to_text: add, covis, erase, clear, reloc, loop,
// score; doubles as hex floats) and writes one line per reloc / loop (the returned keyframes' ids) and per score (the
// double's bits).  GPU.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "KeyFrameDatabase.h"

using namespace ORB_SLAM2;

static DBoW2::BowVector read_bow(std::istringstream& in) {
    DBoW2::BowVector v;
    int n = 0;
    in >> n;
    for (int i = 0; i < n; i++) {
        unsigned w;
        std::string x;
        in >> w >> x;
        v[w] = strtod(x.c_str(), nullptr);
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s script results\n", argv[0]), 2;
    std::ifstream src(argv[1]);
    FILE* dst = fopen(argv[2], "w");
    if (!src || !dst) return fprintf(stderr, "cannot open the files\n"), 2;
    try {
        ORBVocabulary voc;
        KeyFrameDatabase db(voc);
        std::vector<std::unique_ptr<KeyFrame> > kfs;
        std::vector<std::vector<int> > covis;
        long unsigned int next_query = 1000000;
        auto wire = [&]() {
            for (size_t i = 0; i < kfs.size(); i++) {
                kfs[i]->best_covisibles.clear();
                if (i < covis.size())
                    for (int j : covis[i])
                        if ((size_t)j < kfs.size()) kfs[i]->best_covisibles.push_back(kfs[j].get());
            }
        };
        std::string line;
        while (std::getline(src, line)) {
            std::istringstream in(line);
            std::string op;
            if (!(in >> op)) continue;
            if (op == "add") {
                kfs.emplace_back(new KeyFrame());
                kfs.back()->mnId = kfs.size() - 1;
                kfs.back()->mBowVec = read_bow(in);
                db.add(kfs.back().get());
            } else if (op == "covis") {
                int id = 0, m = 0;
                in >> id >> m;
                if ((size_t)id >= covis.size()) covis.resize(id + 1);
                covis[id].resize(m);
                for (int i = 0; i < m; i++) in >> covis[id][i];
            } else if (op == "erase") {
                int id = 0;
                in >> id;
                db.erase(kfs.at(id).get());
            } else if (op == "clear") {
                db.clear();
            } else if (op == "reloc" || op == "loop") {
                std::vector<KeyFrame*> got;
                wire();
                if (op == "reloc") {
                    Frame F;
                    F.mnId = next_query++;
                    F.mBowVec = read_bow(in);
                    got = db.DetectRelocalizationCandidates(&F);
                } else {
                    std::string ms;
                    int nc = 0;
                    in >> ms >> nc;
                    KeyFrame q;
                    q.mnId = next_query++;
                    for (int i = 0; i < nc; i++) {
                        int id = 0;
                        in >> id;
                        q.connected.push_back(kfs.at(id).get());
                    }
                    q.mBowVec = read_bow(in);
                    got = db.DetectLoopCandidates(&q, (float)strtod(ms.c_str(), nullptr));
                }
                fprintf(dst, "%s", op.c_str());
                for (KeyFrame* k : got) fprintf(dst, " %lu", k->mnId);
                fprintf(dst, "\n");
            } else if (op == "score") {
                const DBoW2::BowVector a = read_bow(in), b = read_bow(in);
                const double s = voc.score(a, b);
                uint64_t bits;
                memcpy(&bits, &s, 8);
                fprintf(dst, "score %016" PRIx64 "\n", bits);
            } else {
                return fprintf(stderr, "unknown operation %s\n", op.c_str()), 2;
            }
            if (!in && !in.eof()) return fprintf(stderr, "malformed line: %s\n", line.c_str()), 2;
        }
    } catch (const std::exception& e) {
        fclose(dst);
        return fprintf(stderr, "%s\n", e.what()), 1;
    }
    fclose(dst);
    return 0;
}
