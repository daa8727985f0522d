// Host check of csrc/frame_cell.h (the lines k_frame_grid runs) and of a host model of the kernel's algorithm
// (count, exclusive scan, unordered scatter, per-segment ascending order) against the push-back loop of
// Frame::AssignFeaturesToGrid as orb_features_in_area restates it.  Stand-alone: built with
// -fsanitize=address,undefined and run directly (tests/test_frame_cell_host.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../orb-slam-birdview_amd/csrc/frame_cell.h"

using orbgpu::frame_cell;

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            g_failed++;                                                      \
        }                                                                    \
    } while (0)

static int cell_unit(float x, float y) { return frame_cell(x, y, 0.0f, 0.0f, 1.0f, 1.0f); }

struct Pt {
    float x, y;
};

// the reference: grid[px][py].push_back(i) in index order, with orb_features_in_area's int conversion (the inputs
// here are finite and small, so the conversion is defined)
static void reference_grid(const std::vector<Pt>& p, float min_x, float min_y, float inv_w, float inv_h,
                           std::vector<int>& off, std::vector<int>& idx) {
    std::vector<std::vector<int>> grid(64 * 48);
    for (int i = 0; i < (int)p.size(); i++) {
        const int px = (int)std::round((p[i].x - min_x) * inv_w);
        const int py = (int)std::round((p[i].y - min_y) * inv_h);
        if (px < 0 || px >= 64 || py < 0 || py >= 48) continue;
        grid[px * 48 + py].push_back(i);
    }
    off.assign(64 * 48 + 1, 0);
    idx.clear();
    for (int c = 0; c < 64 * 48; c++) {
        off[c] = (int)idx.size();
        idx.insert(idx.end(), grid[c].begin(), grid[c].end());
    }
    off[64 * 48] = (int)idx.size();
}

// the kernel's algorithm on the host: count per cell, exclusive scan, a scatter in an arbitrary order (here: the
// keypoints visited in a shuffled order, as concurrent lanes would claim slots), then each segment ascending
static void model_grid(const std::vector<Pt>& p, float min_x, float min_y, float inv_w, float inv_h, std::mt19937& rng,
                       std::vector<int>& off, std::vector<int>& idx) {
    const int n = (int)p.size();
    std::vector<int> cell(n), cnt(64 * 48, 0);
    for (int i = 0; i < n; i++) {
        cell[i] = frame_cell(p[i].x, p[i].y, min_x, min_y, inv_w, inv_h);
        if (cell[i] >= 0) cnt[cell[i]]++;
    }
    off.assign(64 * 48 + 1, 0);
    for (int c = 0; c < 64 * 48; c++) off[c + 1] = off[c] + cnt[c];
    std::vector<int> cur(off.begin(), off.end() - 1), tmp(off[64 * 48]), order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    for (int i : order)
        if (cell[i] >= 0) tmp[cur[cell[i]]++] = i;
    idx.assign(off[64 * 48], -1);
    for (int c = 0; c < 64 * 48; c++)
        for (int e = off[c]; e < off[c + 1]; e++) {   // rank = how many of the segment are smaller
            int rank = 0;
            for (int j = off[c]; j < off[c + 1]; j++) rank += tmp[j] < tmp[e];
            idx[off[c] + rank] = tmp[e];
        }
}

int main() {
    // rounding edges: (x - min_x) * inv_w exactly k + 0.5, -0.5, -0.49, 63.49, 63.5; y against 47.5 and 48
    CHECK(cell_unit(0.5f, 0.0f) == 1 * 48);
    CHECK(cell_unit(1.5f, 0.0f) == 2 * 48);
    CHECK(cell_unit(2.5f, 0.0f) == 3 * 48);   // half away from zero, not half to even
    CHECK(cell_unit(62.5f, 0.0f) == 63 * 48);
    CHECK(cell_unit(-0.5f, 0.0f) == -1);
    CHECK(cell_unit(-0.49f, 0.0f) == 0);
    CHECK(cell_unit(-0.3f, -0.3f) == 0);      // -0 lies in cell 0
    CHECK(cell_unit(63.49f, 0.0f) == 63 * 48);
    CHECK(cell_unit(63.5f, 0.0f) == -1);
    CHECK(cell_unit(64.0f, 0.0f) == -1);
    CHECK(cell_unit(0.0f, 0.5f) == 1);
    CHECK(cell_unit(0.0f, -0.5f) == -1);
    CHECK(cell_unit(0.0f, -0.49f) == 0);
    CHECK(cell_unit(0.0f, 47.49f) == 47);
    CHECK(cell_unit(0.0f, 47.5f) == -1);
    CHECK(cell_unit(0.0f, 48.0f) == -1);
    CHECK(cell_unit(63.0f, 47.0f) == 63 * 48 + 47);
    // a scaled grid with an origin: x = min_x + (k + 0.5) / inv_w, exact in float
    CHECK(frame_cell(8.0f + 2 * 0.5f, 4.0f + 2 * 1.0f, 8.0f, 4.0f, 0.5f, 0.5f) == 1 * 48 + 1);
    CHECK(frame_cell(8.0f + 2 * 63.5f, 4.0f, 8.0f, 4.0f, 0.5f, 0.5f) == -1);
    CHECK(frame_cell(8.0f - 2 * 0.5f, 4.0f, 8.0f, 4.0f, 0.5f, 0.5f) == -1);
    // values no int holds: they fall out, and nothing is converted (UBSan would report the conversion)
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (float v : {nan, inf, -inf, 1e30f, -1e30f, 3e9f, -3e9f}) {
        CHECK(cell_unit(v, 1.0f) == -1);
        CHECK(cell_unit(1.0f, v) == -1);
        CHECK(cell_unit(v, v) == -1);
    }
    CHECK(frame_cell(1.0f, 1.0f, 0.0f, 0.0f, 1e38f, 1e38f) == -1);   // the product overflows to inf

    std::mt19937 rng(7);
    std::vector<int> off_r, idx_r, off_m, idx_m;
    {   // 1,000 random keypoints over and around a Frame whose bounds are not the image's
        std::uniform_real_distribution<float> ux(-6.0f, 646.0f), uy(-6.0f, 486.0f);
        std::vector<Pt> p(1000);
        for (auto& q : p) q = Pt{ux(rng), uy(rng)};
        const float min_x = 3.5f, max_x = 636.0f, min_y = 1.0f, max_y = 470.5f;
        const float inv_w = 64.0f / (max_x - min_x), inv_h = 48.0f / (max_y - min_y);
        reference_grid(p, min_x, min_y, inv_w, inv_h, off_r, idx_r);
        model_grid(p, min_x, min_y, inv_w, inv_h, rng, off_m, idx_m);
        CHECK(off_r == off_m);
        CHECK(idx_r == idx_m);
        CHECK(off_r[64 * 48] > 900 && off_r[64 * 48] < 1000);
    }
    {   // 300 keypoints in one cell
        std::uniform_real_distribution<float> u(-3.0f, 3.0f);
        std::vector<Pt> p(300);
        for (auto& q : p) q = Pt{100.0f + u(rng), 200.0f + u(rng)};
        reference_grid(p, 0.0f, 0.0f, 0.1f, 0.1f, off_r, idx_r);
        model_grid(p, 0.0f, 0.0f, 0.1f, 0.1f, rng, off_m, idx_m);
        CHECK(off_r == off_m);
        CHECK(idx_r == idx_m);
        CHECK(off_r[10 * 48 + 20 + 1] - off_r[10 * 48 + 20] == 300);
    }
    if (g_failed) return 1;
    std::printf("frame_cell OK\n");
    return 0;
}
