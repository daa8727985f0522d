// The list-decision rule of the matcher replays (csrc/topk_scan.h) on hand-written lists, K = 8: which entries a
// replay takes from a ranked list, and when the list cannot decide them and has to be ranked again.  Plain host
// C++; built and run by tests/test_topk_scan_host.py.  The expected values restate what the reference's loops keep
// as their running minima when they visit the same candidates (ORBmatcher.cc line numbers beside each case).
#include <cstdio>
#include <vector>

#include "../../orb-slam-birdview_amd/csrc/topk_scan.h"

using orbgpu::kTopkNoStop;
using orbgpu::topk_scan;
using orbgpu::TopkPick;

namespace {
constexpr int K = 8;
int failures = 0;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            failures++;                                                   \
        }                                                                 \
    } while (0)

// Two items, so that the i * K indexing is exercised: item 0 is a decoy whose entries every case would take
// (distance 0, train 1000 + slot), item 1 holds the case's list.
struct Lists {
    std::vector<int> dist, idx, nvalid;
    Lists(std::vector<int> d, std::vector<int> t, int nv) : dist(K, 0), idx(K), nvalid{K, nv} {
        for (int j = 0; j < K; j++) idx[j] = 1000 + j;
        dist.insert(dist.end(), d.begin(), d.end());
        idx.insert(idx.end(), t.begin(), t.end());
    }
    template <class Admit>
    bool scan(int need, Admit admit, int stop_at, TopkPick& p) const {
        return topk_scan(dist.data(), idx.data(), nvalid.data(), K, 1, need, admit, stop_at, p);
    }
};

const std::vector<int> kDist = {3, 5, 7, 9, 11, 13, 15, 17};
const std::vector<int> kTrain = {40, 41, 42, 43, 44, 45, 46, 47};
auto all = [](int, int) { return true; };
auto none = [](int, int) { return false; };

void run_cases() {
    TopkPick p;
    // (a) nothing taken yet: the first two entries are bestDist1 / bestIdx and bestDist2 of every two-minimum loop
    // (SearchByBoW :216-225, SearchForInitialization :447-456); decided whatever nvalid says
    CHECK(Lists(kDist, kTrain, 30).scan(2, all, kTopkNoStop, p));
    CHECK(p.found == 2 && p.d[0] == 3 && p.t[0] == 40 && p.d[1] == 5 && p.t[1] == 41);

    // (b) seven of the window's eight candidates are taken (`if(vpMapPointMatches[realIdxF]) continue;` :209-210):
    // the list holds every candidate (nvalid = 8), so the one left is the best and bestDist2 keeps its initial value
    auto only47 = [](int t, int) { return t == 47; };
    CHECK(Lists(kDist, kTrain, 8).scan(2, only47, kTopkNoStop, p));
    CHECK(p.found == 1 && p.d[0] == 17 && p.t[0] == 47 && p.dist(1, 256) == 256);

    // (c) all eight listed candidates are taken and the item had a ninth (nvalid = 9): the ninth may be admissible
    // and the list does not hold it, so the replay has to rank again (the exhaustion SearchByBoW's vbMatched2 /
    // vpMapPointMatches skip causes, :209-210 / :576-577)
    CHECK(!Lists(kDist, kTrain, 9).scan(2, none, kTopkNoStop, p));
    CHECK(p.found == 0);

    // (c') the common form of it: one admissible entry left, a second wanted for the ratio test (:230 / :461 / :600)
    CHECK(!Lists(kDist, kTrain, 9).scan(2, only47, kTopkNoStop, p));
    CHECK(p.found == 1 && p.t[0] == 47);

    // (d) all eight taken and there were only eight: nothing is admissible, bestDist1 stays at its initial value and
    // the query matches nothing (256 > TH_LOW, :228)
    CHECK(Lists(kDist, kTrain, 8).scan(2, none, kTopkNoStop, p));
    CHECK(p.found == 0 && p.dist(0, 256) == 256 && p.t[0] == -1);

    // (e) a window with three candidates (GetFeaturesInArea returned three, :427-428): the list ends at the
    // terminator, whatever an earlier ranking left behind it is not read, and the list is decided
    auto not40_41 = [](int t, int) { return t != 40 && t != 41; };
    CHECK(Lists({3, 5, 7, -1, 0, 0, 0, 0}, {40, 41, 42, -1, 90, 91, 92, 93}, 3).scan(2, not40_41, kTopkNoStop, p));
    CHECK(p.found == 1 && p.d[0] == 7 && p.t[0] == 42);

    // (f) SearchByProjection(CurrentFrame, LastFrame) keeps one minimum only (bestDist / bestIdx2, :1397-1423):
    // need = 1 stops at the first admissible entry, and is decided although nvalid > K and a second was never looked for
    CHECK(Lists(kDist, kTrain, 30).scan(1, all, 256, p));
    CHECK(p.found == 1 && p.d[0] == 3 && p.t[0] == 40);
    auto not40 = [](int t, int) { return t != 40; };
    CHECK(Lists(kDist, kTrain, 30).scan(1, not40, 256, p));
    CHECK(p.found == 1 && p.d[0] == 5 && p.t[0] == 41);

    // (g) the projection searches start bestDist and bestDist2 at 256 and update on '<' only (:76-78 and :102,
    // :1952-1954 and :1971), so a candidate at distance 256 never becomes a minimum: with stop_at = 256 the scan ends
    // there, decided with one entry although nvalid > K.  The window searches start at INT_MAX (:432-433, :2030-2032),
    // where the same list gives two
    const Lists g({10, 256, 256, 256, 256, 256, 256, 256}, kTrain, 30);
    CHECK(g.scan(2, all, 256, p));
    CHECK(p.found == 1 && p.d[0] == 10 && p.t[0] == 40 && p.dist(1, 256) == 256);
    CHECK(g.scan(2, all, kTopkNoStop, p));
    CHECK(p.found == 2 && p.d[1] == 256 && p.t[1] == 41);

    // (h) `if(vMatchedDistance[i2]<=dist) continue;` (:444-445; vMatchedDistanceBird :2051): admission depends on the
    // entry's own distance.  Train 40 was matched at 3 (equal: skipped), 41 at 4 (closer: skipped), 42 at 8 (this
    // query is closer: a steal), 43 never
    std::vector<int> matched(100, 1 << 30);
    matched[40] = 3;
    matched[41] = 4;
    matched[42] = 8;
    auto closer = [&](int t, int d) { return matched[t] > d; };
    CHECK(Lists(kDist, kTrain, 30).scan(2, closer, kTopkNoStop, p));
    CHECK(p.found == 2 && p.d[0] == 7 && p.t[0] == 42 && p.d[1] == 9 && p.t[1] == 43);
}
}  // namespace

int main() {
    run_cases();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
