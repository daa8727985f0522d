// Host model of the one- and two-frame pyramid (csrc/extract_kernels.hip chain_job and resize_tile), driven by
// tests/test_pyramid_chain_host.py.  For an image size, scale factor and level count it builds the level sizes as
// build_geometry does, the coefficient tables with the library's resize_coefs and the plan with the library's
// build_chain, and walks every job of the plan as chain_job does, thread index by thread index, checking
//   * tiling: the jobs' output tiles reg[level] cover every pixel of every level base+1..top exactly once, the store
//     guard leaves no column unwritten and a dword store never passes the level's pitch;
//   * base load: every load is inside the source image (row < h, byte < w), the dword form only with its four bytes
//     inside the row (the sc1 byte form's containing aligned dword is reported: ld8_outside);
//   * LDS: every byte the value computation selects was written by the previous stage, every access (the third
//     realigned dword included) is below sg.lds_bytes; how far that dword reaches past a region's last row is reported;
//   * coefficients: no read leaves the level's table; coef_entries and buf_bytes bound what each job uses;
//   * values: every pixel equals the plain two-row formula applied level by level from the frame (3.x and generic
//     vertical forms; pseudo-random and all-255 sources).
// It then walks resize_tile for every level (the per-level launches of the small plan and of the fallback, and the
// dataflow launch's resize tasks) with the staging form the source alignment selects and the TH / KP launch_extract
// picks from rs_tiled / rs_chunks (restated here), with the same checks against the source allocation and the LDS
// tile of rs_span_rows * kRsPitch bytes.
//
// usage: chain_model W H scale nlevels first_base seg_len generic align [edit]
//   align 16: frame base and stride multiples of 16; 4: stride a multiple of 4, not of 16; 1: odd stride and base
//   edit (the walk's arithmetic made wrong on purpose, to show the walk notices): hkeep7 | packed8chain |
//   packed8tile | c0c0
// Prints the level sizes, the FAST carve of a wave (the library's fast_wave_layout), the plan ("norplan" when build_chain returns none), per level which kernel, tiling and
// forms the launch takes, and "ok" last; exits 1 with "violation line N" on the first violation.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

static std::string g_edit;
static bool g_gen;

static unsigned umul24(unsigned a, unsigned b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
static unsigned mul_hi_u24(unsigned a, unsigned b) {
    return (unsigned)(((unsigned long long)(a & 0xFFFFFFu) * (b & 0xFFFFFFu)) >> 32);
}
// the plain formula (k_resize's)
static unsigned ref_v(unsigned c0, unsigned c1, unsigned h0, unsigned h1) {
    if (g_gen) {
        const unsigned v = (c0 * h0 + c1 * h1 + (1u << 21)) >> 22;
        return v < 255u ? v : 255u;
    }
    return (((c0 * (h0 >> 4)) >> 16) + ((c1 * (h1 >> 4)) >> 16) + 2) >> 2;
}
// the kernels' form: weights as rs_row_entry leaves them, sums through rs_hkeep, rs_vsum
static unsigned row_w0(const ResizeCoef& c) { return g_gen ? c.c0 : c.c0 << 12; }
static unsigned row_w1(const ResizeCoef& c) { return g_gen ? c.c1 : (g_edit == "c0c0" ? c.c0 : c.c1) << 12; }
static unsigned hkeep(unsigned h) { return g_gen ? h : h & (g_edit == "hkeep7" ? ~7u : ~15u); }
static unsigned vpass(unsigned w0, unsigned w1, unsigned h0, unsigned h1) {
    if (g_gen) {
        const unsigned v = (umul24(w0, h0) + umul24(w1, h1) + (1u << 21)) >> 22;
        return v < 255u ? v : 255u;
    }
    return (mul_hi_u24(w0, hkeep(h0)) + mul_hi_u24(w1, hkeep(h1)) + 2) >> 2;
}

struct Image {
    int w = 0, h = 0, stride = 0, off = 0;   // bytes [off, off + stride * h) of `mem` are the allocation the caller owns
    std::vector<uint8_t> mem;
    uint8_t at(int x, int y) const { return mem[off + (size_t)y * stride + x]; }
};

static int r4(int x) { return (x + 3) & ~3; }

int main(int argc, char** argv) {
    if (argc < 9) return 2;
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]);
    const float scaleFactor = (float)std::atof(argv[3]);
    const int nl = std::atoi(argv[4]), first_base = std::atoi(argv[5]), seg_len = std::atoi(argv[6]);
    g_gen = std::atoi(argv[7]) != 0;
    const int align = std::atoi(argv[8]);
    if (argc > 9) g_edit = argv[9];
    CHECK(nl >= 1 && nl <= ORBGPU_MAX_LEVELS && (align == 16 || align == 4 || align == 1));

    // level sizes (compute_tables, build_geometry) and whether the grids are valid at every level
    static Geom g;
    std::memset(&g, 0, sizeof g);
    g.nlevels = nl;
    g.W = W;
    g.H = H;
    std::vector<ResizeCoef> coefs;
    int off[ORBGPU_MAX_LEVELS] = {0};
    float sc[ORBGPU_MAX_LEVELS];
    sc[0] = 1.0f;
    for (int i = 1; i < nl; i++) sc[i] = (float)(sc[i - 1] * (double)scaleFactor);
    bool valid = W <= kMaxDim && H <= kMaxDim;
    long long pyr = 0;
    std::printf("levels");
    for (int l = 0; l < nl; l++) {
        LevelGeom& L = g.L[l];
        L.w = (int)std::nearbyint((float)W * (1.0f / sc[l]));
        L.h = (int)std::nearbyint((float)H * (1.0f / sc[l]));
        L.pitch = (L.w + 63) & ~63;
        std::printf(" %dx%d", L.w, L.h);
        const float width = (float)(L.w - kEdgeThreshold + 3 - kMinBorder), height = (float)(L.h - kEdgeThreshold + 3 - kMinBorder);
        const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);
        if (nCols <= 0 || nRows <= 0 || L.w < 2 || L.h < 2) valid = false;
        else if ((int)std::ceil(width / nCols) + 6 > kFastMaxRoi || (int)std::ceil(height / nRows) + 6 > kFastMaxRoi ||
                 (int)std::round(width / height) <= 0)
            valid = false;
        if (nCols > 0 && nRows > 0) L.nCols = nCols, L.nRows = nRows, L.wCell = (int)std::ceil(width / nCols), L.hCell = (int)std::ceil(height / nRows);
        if (l == 0) continue;
        L.pyr_off = pyr;
        pyr += (long long)L.pitch * L.h;
        off[l] = (int)coefs.size();
        resize_coefs(g.L[l - 1].w, L.w, coefs, false);
        resize_coefs(g.L[l - 1].h, L.h, coefs, true);
    }
    std::printf("\nvalid %d\n", valid ? 1 : 0);
    // the dataflow launch gives 16 waves a FAST carve each (build_flow: 16 * fast_wave_bytes within a CU's LDS)
    fast_wave_layout(g);
    std::printf("fast_wave_bytes %d\n", g.fast_wave_bytes);
    // rs_tiled / rs_span_rows / rs_chunks as build_geometry derives them
    for (int l = 1; l < nl; l++) {
        LevelGeom& L = g.L[l];
        const ResizeCoef* cx = &coefs[off[l]];
        const ResizeCoef* cy = cx + L.w;
        bool xfits = true;
        for (int x0 = 0; x0 < L.w && xfits; x0 += kRsTileW) {
            const int x1 = std::min(x0 + kRsTileW, L.w) - 1;
            xfits = cx[x1].s1 - (cx[x0].s0 & ~15) + 1 <= kRsPitch;
        }
        int span_rows[2] = {0, 0};
        for (int i = 0; i < 2 && xfits; i++) {
            const int th = 16 << i;
            bool fits = true;
            for (int y0 = 0; y0 < L.h && fits; y0 += th) {
                const int y1 = std::min(y0 + th, L.h) - 1;
                span_rows[i] = std::max(span_rows[i], cy[y1].s1 - cy[y0].s0 + 1);
                fits = cy[y1].s1 - cy[y0].s0 + 1 <= rs_rows(th);
            }
            if (fits) L.rs_tiled |= 1 << i;
        }
        L.rs_span_rows = (L.rs_tiled & 2) ? span_rows[1] : span_rows[0];
        if (L.rs_tiled & 3) {
            const int th = (L.rs_tiled & 2) ? 32 : 16;
            int nq_max = 0, nr_max = 0;
            for (int x0 = 0; x0 < L.w; x0 += kRsTileW) {
                const int x1 = std::min(x0 + kRsTileW, L.w) - 1;
                nq_max = std::max(nq_max, ((cx[x1].s1 - (cx[x0].s0 & ~15)) >> 4) + 1);
            }
            for (int y0 = 0; y0 < L.h; y0 += th) {
                const int y1 = std::min(y0 + th, L.h) - 1;
                nr_max = std::max(nr_max, cy[y1].s1 - cy[y0].s0 + 1);
            }
            L.rs_chunks = nq_max * nr_max;
        }
    }

    std::vector<ChainJob> jobs;
    ChainPlan plan;
    build_chain(g, coefs, off, jobs, plan, first_base, seg_len);
    const int fstride = align == 16 ? (W + 15) & ~15 : align == 4 ? (r4(W) % 16 ? r4(W) : r4(W) + 4) : W | 1;
    const int foff = align == 1 ? 1 : 0;
    std::printf("align %d stride %d base_off %d\n", align, fstride, foff);
    if (!plan.nseg) std::printf("norplan\n");
    else std::printf("plan nseg %d first_base %d\n", plan.nseg, plan.first_base);

    for (int fill = 0; fill < 2; fill++) {
        // the frame (pad bytes 0xA5) and every level by the plain formula
        std::vector<Image> ref(nl);
        ref[0].w = W, ref[0].h = H, ref[0].stride = fstride, ref[0].off = foff;
        ref[0].mem.assign((size_t)fstride * H + foff + 64, 0xA5);
        unsigned rng = 12345u;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                ref[0].mem[foff + (size_t)y * fstride + x] = fill ? 255 : (uint8_t)((rng = rng * 1664525u + 1013904223u) >> 24);
        for (int l = 1; l < nl; l++) {
            Image& D = ref[l];
            const Image& S = ref[l - 1];
            D.w = g.L[l].w, D.h = g.L[l].h, D.stride = g.L[l].pitch;
            D.mem.assign((size_t)D.stride * D.h + 64, 0xA5);
            const ResizeCoef* cx = &coefs[off[l]];
            const ResizeCoef* cy = cx + D.w;
            for (int y = 0; y < D.h; y++)
                for (int x = 0; x < D.w; x++) {
                    const unsigned h0 = S.at(cx[x].s0, cy[y].s0) * (unsigned)cx[x].c0 + S.at(cx[x].s1, cy[y].s0) * (unsigned)cx[x].c1;
                    const unsigned h1 = S.at(cx[x].s0, cy[y].s1) * (unsigned)cx[x].c0 + S.at(cx[x].s1, cy[y].s1) * (unsigned)cx[x].c1;
                    D.mem[(size_t)y * D.stride + x] = (uint8_t)ref_v(cy[y].c0, cy[y].c1, h0, h1);
                }
        }

        /* ---------------- chain_job over every job of the plan ---------------- */
        for (int sgi = 0; sgi < plan.nseg; sgi++) {
            const ChainSegment& sg = plan.seg[sgi];
            CHECK(sg.njobs > 0 && sg.lds_bytes == 2 * sg.buf_bytes + 16 * sg.coef_entries && sg.lds_bytes <= 64 * 1024);
            CHECK(sg.buf_bytes % 16 == 0);
            const int base = jobs[sg.job0].base, top = jobs[sg.job0 + sg.njobs - 1].level;
            int used_buf = 0, used_coef = 0;
            std::vector<std::vector<int>> cover(nl), stored(nl);
            for (int l = base + 1; l <= top; l++) {
                cover[l].assign((size_t)g.L[l].w * g.L[l].h, 0);
                stored[l].assign((size_t)g.L[l].pitch * g.L[l].h, 0);
            }
            // per stage level: dword groups in the packed form / the byte form; per base load: dwords / byte groups
            std::vector<long long> n_packed(nl, 0), n_bytes(nl, 0);
            long long base_dw = 0, base_by = 0;
            std::vector<int> over3(nl, -1000);
            int ld8_outside = 0;
            const Image& B = ref[base];
            const bool al = ((B.off | B.stride) & 3) == 0;
            std::vector<uint8_t> lds(sg.lds_bytes), wr(sg.lds_bytes);
            for (int j = sg.job0; j < sg.job0 + sg.njobs; j++) {
                const ChainJob& J = jobs[j];
                const int l = J.level, b = J.base;
                CHECK(b == base && l > b && l <= top && l < nl);
                {   // the job's own tile: inside the level, counted once per pixel
                    const int4 R = J.reg[l];
                    const int TW = l - b <= 2 ? 64 : 32, TH = l - b <= 2 ? 32 : 16;
                    CHECK(R.x % TW == 0 && R.z % TH == 0 && R.x < g.L[l].w && R.z < R.w && R.w <= g.L[l].h);
                    for (int y = R.z; y < R.w; y++)
                        for (int x = R.x; x < std::min(R.y, g.L[l].w); x++) cover[l][(size_t)y * g.L[l].w + x]++;
                }
                const size_t buf0 = 0, buf1 = sg.buf_bytes, scb = 2 * (size_t)sg.buf_bytes;
                std::vector<int4> scv(sg.coef_entries, make_int4(0, 0, 0, 0));
                std::vector<uint8_t> scw(sg.coef_entries, 0);
                std::fill(wr.begin(), wr.end(), 0);
                int e0 = 0;
                for (int k = b + 1; k <= l; k++) {
                    const int4 R = J.reg[k], S = J.reg[k - 1];
                    const int nx = R.y - R.x, ny = R.w - R.z, sp = r4(S.y - S.x), wk = g.L[k].w, hk = g.L[k].h;
                    CHECK(nx > 0 && ny > 0 && nx % 4 == 0 && R.x % 4 == 0 && R.x >= 0 && R.z >= 0);
                    const ResizeCoef* cx = &coefs[off[k]];
                    for (int tid = 0; tid < 256; tid++)
                        for (int e = tid; e < nx + ny; e += 256) {
                            int4 v;
                            if (e < nx) {
                                const int i = std::min(R.x + e, wk - 1);
                                CHECK(i >= 0 && i < wk);
                                const ResizeCoef c = cx[i];
                                v = make_int4(c.s0 - S.x, c.s1 - S.x, c.c0, c.c1);
                            } else {
                                const int i = R.z + (e - nx);
                                CHECK(i >= 0 && i < hk);   // the row table has hk entries after the wk columns
                                const ResizeCoef c = cx[wk + i];
                                v = make_int4((c.s0 - S.z) * sp, (c.s1 - S.z) * sp, (int)row_w0(c), (int)row_w1(c));
                            }
                            CHECK(e0 + e < sg.coef_entries && scb + 16 * (size_t)(e0 + e + 1) <= (size_t)sg.lds_bytes);
                            scv[e0 + e] = v;
                            scw[e0 + e] = 1;
                        }
                    e0 += nx + ny;
                }
                used_coef = std::max(used_coef, e0);
                {   // the base region
                    const int4 R = J.reg[b];
                    const int p0 = r4(R.y - R.x), nq = p0 >> 2, ny = R.w - R.z, wb = g.L[b].w, hb = g.L[b].h;
                    CHECK(R.x % 4 == 0 && R.x >= 0 && R.y <= wb && R.z >= 0 && R.w <= hb && p0 * ny <= sg.buf_bytes);
                    used_buf = std::max(used_buf, p0 * ny);
                    const int QW = nq <= 16 ? 16 : nq <= 32 ? 32 : 64, RP = 256 / QW;
                    std::vector<int> seen((size_t)nq * ny, 0);
                    for (int tid = 0; tid < 256; tid++)
                        for (int qb = 0; qb < nq; qb += QW)
                            for (int r = tid / QW; r < ny; r += RP) {
                                const int q = qb + (tid & (QW - 1));
                                if (q >= nq) continue;
                                const int col = R.x + 4 * q, row = R.z + r;
                                CHECK(row < hb && !seen[(size_t)r * nq + q]++);
                                uint8_t v[4] = {0, 0, 0, 0};
                                if (al && col + 3 < wb) {
                                    CHECK((B.off + (long long)row * B.stride + col) % 4 == 0);
                                    for (int t = 0; t < 4; t++) v[t] = B.at(col + t, row);
                                    base_dw++;
                                } else {
                                    for (int t = 0; t < 4; t++)
                                        if (col + t < wb) {
                                            v[t] = B.at(col + t, row);
                                            // the sc1 form loads the byte's aligned dword: how far outside the allocation
                                            const long long a = B.off + (long long)row * B.stride + col + t, d = a & ~3LL;
                                            const long long lo = B.off, hi = B.off + (long long)B.stride * hb;
                                            CHECK(d >= (lo & ~3LL) && d + 4 <= ((hi + 3) & ~3LL));
                                            ld8_outside = std::max(ld8_outside, (int)std::max(lo - d, d + 4 - hi));
                                        }
                                    base_by++;
                                }
                                const size_t a = buf0 + (size_t)r * p0 + 4 * q;
                                CHECK(a + 4 <= (size_t)sg.buf_bytes);
                                for (int t = 0; t < 4; t++) lds[a + t] = v[t], wr[a + t] = 1;
                            }
                    for (int s : seen) CHECK(s == 1);
                }
                e0 = 0;
                for (int k = b + 1; k <= l; k++) {
                    const int4 R = J.reg[k], S = J.reg[k - 1];
                    const int nx = R.y - R.x, ny = R.w - R.z, nq = nx >> 2, sp = r4(S.y - S.x), srows = S.w - S.z;
                    const size_t src = ((k - b) & 1) ? buf0 : buf1, dst = ((k - b) & 1) ? buf1 : buf0;
                    const bool last = k == l;
                    const int gpitch = g.L[k].pitch, wk = g.L[k].w;
                    if (!last) {
                        CHECK(nx * ny <= sg.buf_bytes);
                        used_buf = std::max(used_buf, nx * ny);
                        std::fill(wr.begin() + dst, wr.begin() + dst + sg.buf_bytes, 0);   // two stages old: not this stage's
                    }
                    const int QW = nq <= 16 ? 16 : nq <= 32 ? 32 : 64, RP = 256 / QW;
                    for (int tid = 0; tid < 256; tid++)
                        for (int qb = 0; qb < nq; qb += QW) {
                            const int q = qb + (tid & (QW - 1));
                            if (q >= nq) continue;
                            int o0[4], o1[4];
                            unsigned c0[4], c1[4];
                            for (int t = 0; t < 4; t++) {
                                CHECK(4 * q + t < nx && scw[e0 + 4 * q + t]);
                                const int4 cx = scv[e0 + 4 * q + t];
                                o0[t] = cx.x, o1[t] = cx.y, c0[t] = cx.z, c1[t] = cx.w;
                                CHECK(o0[t] >= 0 && o1[t] >= o0[t] && o1[t] < sp);
                            }
                            const int bo = o0[0], bw = bo >> 2;
                            const bool packed_ok = o1[3] - bo <= (g_edit == "packed8chain" ? 8 : 7);
                            if (tid / QW == 0) (packed_ok ? n_packed : n_bytes)[k]++;
                            for (int r = tid / QW; r < ny; r += RP) {
                                CHECK(scw[e0 + nx + r]);
                                const int4 cy = scv[e0 + nx + r];
                                CHECK(cy.x >= 0 && cy.y >= cy.x && cy.y / sp < srows && cy.x % sp == 0 && cy.y % sp == 0);
                                uint8_t px[4];
                                for (int t = 0; t < 4; t++) {
                                    if (packed_ok) {
                                        // 3 dwords from the aligned one: all inside the carve; the v_perm selects 0..7 of
                                        // the 8 bytes from bo
                                        CHECK(src + cy.y + 4 * bw + 12 <= (size_t)sg.lds_bytes);
                                        CHECK(o0[t] - bo >= 0 && o1[t] - bo <= 7);
                                        over3[k] = std::max(over3[k], cy.y + 4 * bw + 12 - sp * srows);
                                    }
                                    const size_t a00 = src + cy.x + o0[t], a01 = src + cy.x + o1[t];
                                    const size_t a10 = src + cy.y + o0[t], a11 = src + cy.y + o1[t];
                                    CHECK(a11 < src + (size_t)sg.buf_bytes && wr[a00] && wr[a01] && wr[a10] && wr[a11]);
                                    const unsigned h0 = umul24(lds[a00], c0[t]) + umul24(lds[a01], c1[t]);
                                    const unsigned h1 = umul24(lds[a10], c0[t]) + umul24(lds[a11], c1[t]);
                                    CHECK(h0 < (1u << 19) && h1 < (1u << 19));   // mul_hi_u24's operand bound
                                    const unsigned v = vpass((unsigned)cy.z, (unsigned)cy.w, h0, h1);
                                    CHECK(v <= 255u);   // rs_vsum's or-ed pack assumes a byte
                                    px[t] = (uint8_t)v;
                                }
                                if (!last) {
                                    const size_t a = dst + (size_t)r * nx + 4 * q;
                                    CHECK(a + 4 <= dst + (size_t)sg.buf_bytes);
                                    for (int t = 0; t < 4; t++) lds[a + t] = px[t], wr[a + t] = 1;
                                } else if (R.x + 4 * q < wk) {
                                    CHECK(R.x + 4 * q + 4 <= gpitch && R.z + r < g.L[k].h);
                                    for (int t = 0; t < 4; t++) {
                                        const int x = R.x + 4 * q + t, y = R.z + r;
                                        CHECK(!stored[k][(size_t)y * gpitch + x]++);
                                        if (x < wk) CHECK(px[t] == ref[k].at(x, y));
                                    }
                                }
                                // an intermediate region's pixels inside the level are the level's pixels too
                                if (!last)
                                    for (int t = 0; t < 4; t++)
                                        if (R.x + 4 * q + t < wk) CHECK(px[t] == ref[k].at(R.x + 4 * q + t, R.z + r));
                            }
                        }
                    e0 += nx + ny;
                }
            }
            for (int l = base + 1; l <= top; l++) {
                for (int c : cover[l]) CHECK(c == 1);
                for (int y = 0; y < g.L[l].h; y++)
                    for (int x = 0; x < g.L[l].w; x++) CHECK(stored[l][(size_t)y * g.L[l].pitch + x] == 1);
            }
            CHECK(used_buf <= sg.buf_bytes && used_coef == sg.coef_entries && sg.buf_bytes - used_buf < 16);
            if (fill) continue;
            std::printf("seg %d base %d top %d njobs %d buf_bytes %d coef_entries %d lds_bytes %d base_dwords %lld base_bytegroups %lld ld8_outside %d\n",
                        sgi, base, top, sg.njobs, sg.buf_bytes, sg.coef_entries, sg.lds_bytes, base_dw, base_by, ld8_outside);
            for (int l = base + 1; l <= top; l++) {
                const int TW = l - base <= 2 ? 64 : 32, TH = l - base <= 2 ? 32 : 16;
                const int lw = g.L[l].w - (g.L[l].w - 1) / TW * TW, lh = g.L[l].h - (g.L[l].h - 1) / TH * TH;
                std::printf("chain level %d tile %dx%d w %d h %d lastw %d lasth %d packed %lld bytes %lld over3rd %d\n", l, TW,
                            TH, g.L[l].w, g.L[l].h, lw, lh, n_packed[l], n_bytes[l], over3[l]);
            }
        }

        /* ---------------- resize_tile (or k_resize) over every level ---------------- */
        for (int l = 1; l < nl; l++) {
            const LevelGeom& L = g.L[l];
            const Image& S = ref[l - 1];
            const ResizeCoef* coef = &coefs[off[l]];
            const int dw = L.w, dh = L.h, pitch = L.pitch;
            if (!(L.rs_tiled & 3)) {
                // k_resize: a thread's dword at x0 = 4 i < dw stays inside the pitch; the values are the formula itself
                CHECK(((dw - 1) & ~3) + 4 <= pitch);
                if (!fill) std::printf("resize level %d kernel k_resize\n", l);
                continue;
            }
            const int TH = (L.rs_tiled & 2) ? 32 : 16;
            const int kp = L.rs_chunks <= 512 ? 2 : L.rs_chunks <= 768 ? 3 : 0;
            const int KP = TH == 32 ? kp : (kp == 2 ? 2 : 0);
            const int kRows = rs_rows(TH), kQ = kRsPitch / 16;
            const int kPer = KP > 0 ? KP : (kRows * kQ + 255) / 256;
            const size_t alloc = (size_t)L.rs_span_rows * kRsPitch;
            CHECK(L.rs_span_rows <= kRows);
            const bool vec16 = ((S.off | S.stride) & 15) == 0, vec4 = ((S.off | S.stride) & 3) == 0;
            std::vector<uint8_t> lds(alloc), st(alloc);
            std::vector<int> stored((size_t)pitch * dh, 0);
            int over3 = -1000, tiles_packed = 0, tiles_bytes = 0;
            for (int by = 0; by * TH < dh; by++)
                for (int bx = 0; bx * kRsTileW < dw; bx++) {
                    const int x0 = bx * kRsTileW, y0 = by * TH;
                    const int nx = std::min(kRsTileW, dw - x0), ny = std::min(TH, dh - y0);
                    const int sx0 = coef[x0].s0 & (vec16 ? ~15 : ~3), sx1 = coef[x0 + nx - 1].s1;
                    const int sy0 = coef[dw + y0].s0, sy1 = coef[dw + y0 + ny - 1].s1;
                    const int nr = sy1 - sy0 + 1;
                    CHECK(nr >= 1 && nr <= L.rs_span_rows && sx1 - sx0 + 1 <= kRsPitch);
                    const long long lo = S.off, hi = S.off + (long long)S.stride * S.h;
                    const long long base = S.off + (long long)sy0 * S.stride + sx0;
                    std::fill(st.begin(), st.end(), 0);
                    if (vec16) {
                        const int nq = ((sx1 - sx0) >> 4) + 1, total = nr * nq;
                        CHECK(nq >= 1 && nq <= 17 && total <= 256 * kPer && total <= 256 * ((kRows * kQ + 255) / 256));
                        const unsigned magic = (65536u + nq - 1) / nq;   // kRsMagic[nq]
                        for (int tid = 0; tid < 256; tid++)
                            for (int k = 0; k < kPer; k++) {
                                const int i = std::min(tid + 256 * k, total - 1);
                                const int r = (int)(umul24((unsigned)i, magic) >> 16), q = i - r * nq;
                                CHECK(r == i / nq && q >= 0 && q < nq && r < nr);
                                const long long a = base + (long long)r * S.stride + 16 * q;
                                CHECK(a >= lo && a + 16 <= hi && a % 16 == 0);
                                const size_t d = (size_t)r * kRsPitch + 16 * q;
                                CHECK(d + 16 <= alloc);
                                for (int t = 0; t < 16; t++) {
                                    CHECK(!st[d + t] || lds[d + t] == S.mem[a + t]);   // a clamped duplicate: the same bytes
                                    lds[d + t] = S.mem[a + t], st[d + t] = 1;
                                }
                            }
                    } else if (vec4) {
                        const int nw = (sx1 - sx0 + 4) >> 2;
                        CHECK(nw <= 68);
                        for (int i = 0; i < nr * 68; i++) {
                            const int r = i / 68, wd = i - r * 68;
                            if (wd >= nw) continue;
                            const long long a = base + (long long)r * S.stride + 4 * wd;
                            CHECK(a >= lo && a + 4 <= hi && a % 4 == 0);
                            const size_t d = (size_t)r * kRsPitch + 4 * wd;
                            CHECK(d + 4 <= alloc);
                            for (int t = 0; t < 4; t++) lds[d + t] = S.mem[a + t], st[d + t] = 1;
                        }
                    } else {
                        const int nb = sx1 - sx0 + 1;
                        for (int i = 0; i < nr * kRsPitch; i++) {
                            const int r = i / kRsPitch, b = i - r * kRsPitch;
                            if (b >= nb) continue;
                            const long long a = base + (long long)r * S.stride + b;
                            CHECK(a >= lo && a < hi);
                            CHECK((size_t)i < alloc);
                            lds[i] = S.mem[a], st[i] = 1;
                        }
                    }
                    // the wave's ballot: the tile takes the packed form when every active lane's bytes allow it
                    bool all_packed = true;
                    for (int tx = 0; tx < nx; tx += 4) {
                        const int bo = coef[x0 + std::min(tx, nx - 1)].s0 - sx0;
                        const int o13 = coef[x0 + std::min(tx + 3, nx - 1)].s1 - sx0;
                        all_packed = all_packed && o13 - bo <= (g_edit == "packed8tile" ? 8 : 7);
                    }
                    (all_packed ? tiles_packed : tiles_bytes)++;
                    for (int tid = 0; tid < 256; tid++) {
                        const int tx = (tid & 31) * 4;
                        if (tx >= nx) continue;
                        int o0[4], o1[4];
                        unsigned c0[4], c1[4];
                        for (int i = 0; i < 4; i++) {
                            const ResizeCoef c = coef[x0 + std::min(tx + i, nx - 1)];   // s_cx[tx + i]: the clamped entry
                            CHECK(x0 + std::min(tx + i, nx - 1) < dw);
                            o0[i] = c.s0 - sx0, o1[i] = c.s1 - sx0, c0[i] = c.c0, c1[i] = c.c1;
                            CHECK(o0[i] >= 0 && o1[i] < kRsPitch);
                        }
                        const int bo = o0[0], bw = bo >> 2;
                        for (int pass = 0; pass < TH / 8; pass++) {
                            const int ty = pass * 8 + (tid >> 5);
                            if (ty >= ny) break;
                            const ResizeCoef rc = coef[dw + y0 + std::min(ty, ny - 1)];
                            const int cyx = (rc.s0 - sy0) * kRsPitch, cyy = (rc.s1 - sy0) * kRsPitch;
                            CHECK(cyx >= 0 && rc.s1 - sy0 < nr);
                            uint8_t px[4];
                            for (int i = 0; i < 4; i++) {
                                if (all_packed) {
                                    CHECK((size_t)cyy + 4 * bw + 12 <= alloc);
                                    CHECK(o0[i] - bo >= 0 && o1[i] - bo <= 7);
                                    over3 = std::max(over3, cyy + 4 * bw + 12 - nr * kRsPitch);
                                }
                                const size_t a00 = cyx + o0[i], a01 = cyx + o1[i], a10 = cyy + o0[i], a11 = cyy + o1[i];
                                CHECK(a11 < alloc && st[a00] && st[a01] && st[a10] && st[a11]);
                                const unsigned h0 = umul24(lds[a00], c0[i]) + umul24(lds[a01], c1[i]);
                                const unsigned h1 = umul24(lds[a10], c0[i]) + umul24(lds[a11], c1[i]);
                                const unsigned v = vpass(row_w0(rc), row_w1(rc), h0, h1);
                                CHECK(v <= 255u);
                                px[i] = (uint8_t)v;
                            }
                            CHECK(x0 + tx + 4 <= pitch && y0 + ty < dh);
                            for (int i = 0; i < 4; i++) {
                                const int x = x0 + tx + i, y = y0 + ty;
                                CHECK(!stored[(size_t)y * pitch + x]++);
                                if (x < dw) CHECK(px[i] == ref[l].at(x, y));
                            }
                        }
                    }
                }
            for (int y = 0; y < dh; y++)
                for (int x = 0; x < dw; x++) CHECK(stored[(size_t)y * pitch + x] == 1);
            if (!fill)
                std::printf("resize level %d kernel k_resize_tiled TH %d KP %d rs_chunks %d staging %s tiles_packed %d tiles_bytes %d over3rd %d\n",
                            l, TH, KP, L.rs_chunks, vec16 ? "vec16" : vec4 ? "dword" : "byte", tiles_packed, tiles_bytes, over3);
        }
    }
    std::printf("ok\n");
    return 0;
}
