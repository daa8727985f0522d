// The list-decision rule of the matcher replays (matcher.hip), as plain C++: no HIP, no context.
//
// The ranking kernels give every item (query) a list of its K best admissible candidates in (distance, position)
// order, the order of the reference's strict-'<' updates of its running minima: dist[i K + j] and idx[i K + j], a
// list shorter than K ended by a negative distance, and nvalid[i], the number of admissible candidates the item had
// (so the list holds min(nvalid[i], K) entries).  A replay admits fewer candidates than the kernel did, because
// matches accepted since the ranking take trains away; what the reference's loop would have kept as its best and
// second best are then the first one or two entries of the list that are still admissible.
#pragma once
#include <climits>
#include <cstddef>

namespace orbgpu {

constexpr int kTopkNoStop = INT_MAX;   // a stop_at no distance reaches

struct TopkPick {
    int found = 0;      // entries taken, at most `need`
    int d[2] = {0, 0};  // their distances and trains, [0] the best; [k] means something for k < found only
    int t[2] = {-1, -1};
    int dist(int k, int init) const { return k < found ? d[k] : init; }   // (a running minimum nothing updated)
};

// The first `need` (1 or 2) entries of item i's list that admit(train, distance) accepts.  An entry with a distance
// of stop_at or more ends the scan: no later entry can update a minimum that starts at stop_at.  Returns whether
// the list decided them: it gave `need` entries, or it ended (terminator or stop_at), or it holds every candidate
// the item had (nvalid[i] <= K).  Otherwise candidates beyond the list may be admissible, and the caller re-ranks.
// A terminator decides on the kernels' invariant that a list holds min(nvalid[i], K) entries: one that ends before
// slot K has nvalid[i] < K, so nothing lies beyond it.
template <class Admit>
bool topk_scan(const int* dist, const int* idx, const int* nvalid, int K, int i, int need, Admit admit, int stop_at,
               TopkPick& p) {
    p = TopkPick{};
    for (int j = 0; j < K; j++) {
        const int d = dist[(size_t)i * K + j];
        if (d < 0 || d >= stop_at) return true;
        const int t = idx[(size_t)i * K + j];
        if (!admit(t, d)) continue;
        if (p.found == 0) {   // (constant indices: p stays in registers once this is inlined into a replay)
            p.d[0] = d;
            p.t[0] = t;
            p.found = 1;
            if (need == 1) return true;
        } else {
            p.d[1] = d;
            p.t[1] = t;
            p.found = 2;
            return true;
        }
    }
    return nvalid[i] <= K;
}

}  // namespace orbgpu
