// Host model of k_resize_rows (csrc/extract_kernels.hip), driven by tests/test_resize_rows_host.py: for a level
// size and scale factor it takes the library's own coefficient tables (resize_coefs) and launch geometry
// (rr_geometry) and walks every block, wave and lane the way the kernel does, checking
//   * the block -> tile map (XCD-local order, recip20 row split) is a bijection onto the tiles;
//   * every staged chunk lies inside the source image and inside the LDS tile the launch allocates;
//   * every LDS dword a lane reads lies inside that tile and was staged or is padding of a staged row;
//   * the strip walk (kept row, fresh pass when the upper row is not the kept one) produces, for every output
//     pixel, the value of the plain two-row formula (k_resize's), 3.x and generic forms.
// Prints "ok <tiles> <rows> <pitch>" or "untiled" (rr_geometry refuses the level); exits 1 on a violation.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../orb-slam-birdview_amd/csrc/orbgpu_internal.h"

using namespace orbgpu;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("violation line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

static unsigned vsum(bool gen, unsigned c0, unsigned c1, unsigned h0, unsigned h1) {
    if (gen) {
        const unsigned v = (c0 * h0 + c1 * h1 + (1u << 21)) >> 22;
        return v < 255u ? v : 255u;
    }
    return (((c0 * (h0 >> 4)) >> 16) + ((c1 * (h1 >> 4)) >> 16) + 2) >> 2;
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const int sw = std::atoi(argv[1]), sh = std::atoi(argv[2]), dw = std::atoi(argv[3]), dh = std::atoi(argv[4]);
    const bool gen = std::atoi(argv[5]) != 0;
    std::vector<ResizeCoef> coef;
    resize_coefs(sw, dw, coef, false);
    resize_coefs(sh, dh, coef, true);
    const ResizeCoef* cx = coef.data();
    const ResizeCoef* cy = cx + dw;
    const RrGeom rr = rr_geometry(cx, dw, cy, dh);
    if (!rr.rows) {
        std::printf("untiled\n");
        return 0;
    }
    const int stride = (sw + 63) & ~63, lp = rr.pitch, KP = rr.rows <= 48 ? 6 : kRrMaxRows / 8;
    CHECK(rr.rows <= 8 * KP && lp % 16 == 0);
    std::vector<uint8_t> src((size_t)stride * sh), out((size_t)dw * dh, 0), ref((size_t)dw * dh);
    unsigned rng = 12345u;
    for (auto& b : src) b = (uint8_t)((rng = rng * 1664525u + 1013904223u) >> 24);
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            const uint8_t *r0 = &src[(size_t)cy[y].s0 * stride], *r1 = &src[(size_t)cy[y].s1 * stride];
            const unsigned h0 = r0[cx[x].s0] * (unsigned)cx[x].c0 + r0[cx[x].s1] * (unsigned)cx[x].c1;
            const unsigned h1 = r1[cx[x].s0] * (unsigned)cx[x].c0 + r1[cx[x].s1] * (unsigned)cx[x].c1;
            ref[(size_t)y * dw + x] = (uint8_t)vsum(gen, cy[y].c0, cy[y].c1, h0, h1);
        }
    const int gx = (dw + kRrTileW - 1) / kRrTileW, gy = (dh + kRrTileH - 1) / kRrTileH, nb = gx * gy;
    const unsigned gxRecip = recip20((uint32_t)gx);
    std::vector<int> seen(nb, 0);
    std::vector<uint8_t> lds((size_t)rr.rows * lp), staged((size_t)rr.rows * lp);
    for (int b = 0; b < nb; b++) {
        const int bq = nb >> 3, br = nb & 7, xcd = b & 7, bj = b >> 3;
        const int tile = (xcd < br ? xcd * (bq + 1) : br * (bq + 1) + (xcd - br) * bq) + bj;
        CHECK(tile >= 0 && tile < nb && !seen[tile]++);
        const int by = (int)(((unsigned)tile * gxRecip) >> 20), bx = tile - by * gx;
        CHECK(by == tile / gx && bx >= 0 && bx < gx);
        const int x0 = bx * kRrTileW, y0 = by * kRrTileH;
        const int nx = std::min(kRrTileW, dw - x0), ny = std::min(kRrTileH, dh - y0);
        const int sx0 = cx[x0].s0 & ~15, sx1 = cx[x0 + nx - 1].s1, sy0 = cy[y0].s0, sy1 = cy[y0 + ny - 1].s1;
        const int nr = sy1 - sy0 + 1, nq = ((sx1 - sx0) >> 4) + 1;
        CHECK(nr >= 1 && nr <= rr.rows && nq >= 1 && nq <= kRrMaxChunks);
        const long long records = (long long)(nr - 1) * stride + 16 * nq;
        std::fill(staged.begin(), staged.end(), 0);
        for (int tid = 0; tid < 256; tid++) {
            const int sq = tid & 31, sr = tid >> 5;
            for (int k = 0; k < KP; k++) {
                const long long off = sq < nq ? (long long)(sr + 8 * k) * stride + 16 * sq : 0x40000000LL + 8 * k * stride;
                const bool inrange = off + 16 <= records, stored = sq < nq && sr + 8 * k < nr;
                CHECK(inrange == stored);   // what the range check lets through is what the kernel stores
                if (!stored) continue;
                const long long g = (long long)(sy0 + sr + 8 * k) * stride + sx0 + 16 * sq;
                CHECK(g >= 0 && g + 16 <= (long long)src.size());
                const size_t l = (size_t)(sr + 8 * k) * lp + 16 * sq;
                CHECK(l + 16 <= lds.size());
                for (int i = 0; i < 16; i++) lds[l + i] = src[g + i], staged[l + i] = 1;
            }
        }
        for (int wv = 0; wv < 4; wv++)
            for (int lane = 0; lane < 64; lane++) {
                const int tx = lane * 4, ys = y0 + wv * kRrStrip;
                if (tx >= nx || ys >= y0 + ny) continue;
                ResizeCoef c[4];
                for (int i = 0; i < 4; i++) c[i] = cx[std::min(x0 + tx + i, dw - 1)];
                const int bo = c[0].s0 - sx0;
                CHECK(bo >= 0);
                auto hpass = [&](unsigned (&h)[4], int srow, bool& ok) {
                    const size_t a = (size_t)(srow - sy0) * lp + (bo & ~3);
                    ok = srow >= sy0 && srow <= sy1 && a + 12 <= lds.size() && (bo & ~3) + 12 <= lp;
                    if (!ok) return;
                    uint8_t w[8];   // the 3 dwords realigned to bo: 8 bytes from bo
                    for (int i = 0; i < 8; i++) w[i] = lds[a + (bo & 3) + i];
                    for (int i = 0; i < 4; i++) {
                        const int o0 = c[i].s0 - sx0 - bo, o1 = c[i].s1 - sx0 - bo;
                        ok = ok && o0 >= 0 && o1 <= 7 && staged[a + (bo & 3) + o0] && staged[a + (bo & 3) + o1];
                        if (!ok) return;
                        const unsigned s = w[o0] * (unsigned)c[i].c0 + w[o1] * (unsigned)c[i].c1;
                        h[i] = gen ? s : s & ~15u;
                    }
                };
                unsigned hc[4] = {0, 0, 0, 0}, hn[4];
                int cur = -1;
                for (int k = 0; k < kRrStrip; k++) {
                    if (ys + k >= y0 + ny) break;
                    const ResizeCoef r = cy[std::min(ys + k, dh - 1)];
                    bool ok = true;
                    if (r.s0 != cur) hpass(hc, r.s0, ok);
                    CHECK(ok);
                    hpass(hn, r.s1, ok);
                    CHECK(ok);
                    for (int i = 0; i < 4; i++) {
                        const unsigned v = gen ? vsum(true, r.c0, r.c1, hc[i], hn[i])
                                               : ((unsigned)(((unsigned long long)(r.c0 << 12) * hc[i]) >> 32) +
                                                  (unsigned)(((unsigned long long)(r.c1 << 12) * hn[i]) >> 32) + 2) >> 2;
                        CHECK(v <= 255u);
                        if (x0 + tx + i < dw) out[(size_t)(ys + k) * dw + x0 + tx + i] = (uint8_t)v;
                    }
                    for (int i = 0; i < 4; i++) hc[i] = hn[i];
                    cur = r.s1;
                }
            }
    }
    for (int t = 0; t < nb; t++) CHECK(seen[t] == 1);
    CHECK(out == ref);
    std::printf("ok %d %d %d\n", nb, rr.rows, lp);
    return 0;
}
