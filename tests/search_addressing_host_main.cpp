// Stand-alone host program for csrc/mvx_analyse_addr.h (test infrastructure; tests/test_search_addressing.py builds it at test time with
// AddressSanitizer and UBSan and feeds it the level tables of mvx_analyse_debug_level).  It audits the reference addressing of the search
// kernels that form "64-bit level base + unsigned 32-bit offset": for every level and block of a geometry it forms the legal rectangle, the
// vectors the reference can LOAD there -- the zero vector unconditionally, the corners and edge midpoints of the rectangle, and what the clip
// min(max(v, nDxMin), nDxMax - 1) makes of (0, 0) and of vectors far outside on every side (a clipped global / hierarchical / left / up /
// ahead predictor; on an empty rectangle that is nDxMax - 1 < nDxMin) -- and checks every piece address a kernel family forms from the header's
// unsigned arithmetic against the signed 64-bit truth: base + (u32 offset) must EQUAL the true address as a 64-bit sum, for every row, and the
// bytes read must lie inside [plane start, plane start + the bytes the layout promises).
//
// input (stdin), per geometry:  G name bps chroma blk overlap route range0 range1 nlevels   then nlevels lines  L <the 24 numbers of a level>
// route: 2 the lean / speculative kernels and the specialised general kernels can run it, 1 the specialised general kernels only, 0 generic.
// output: per level "level NAME L emptyx=N emptyy=N blocks=N", then "ok NAME accesses=N" or the first "VIOLATION ..." of the geometry.
// exit status 1 if any geometry has a violation.  Built with -DMVX_REF_BIAS_ROWS=0 -DMVX_REF_BIAS_COLS=0 it audits the arithmetic as it was
// before the bias.  A running offset (po += step) and the direct form (off + row * pitch + xb) are the same number modulo 2^32 whatever the
// stride, so every piece is checked once, from a running offset that advances row by row.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "mvx_analyse_addr.h"

struct Level { int64_t v[24]; };
struct Geo {
    std::string name;
    int bps, chroma, blk, ov, route;
    int64_t range[2];
    std::vector<Level> lv;
};
struct Where { const Geo *g; int level, bx, by, vx, vy; };

static long long g_accesses;
static bool g_bad;

// one access: `bytes` bytes at base + (u32) off of plane `plane`; all positions relative to the plane's first byte
static void check(const Where &w, const char *family, const char *what, int plane, int row, int xb, int64_t base, unsigned off, int64_t truth, int bytes) {
    g_accesses++;
    if (g_bad) return;
    const int64_t got = base + (int64_t)(uint64_t)off;
    const int64_t range = w.g->range[plane ? 1 : 0];
    if (got == truth && truth >= 0 && truth + bytes <= range) return;
    g_bad = true;
    printf("VIOLATION geometry=%s level=%d block=(%d,%d) vector=(%d,%d) family=%s piece=%s plane=%d row=%d xb=%d offset32=%u address=%lld true=%lld diff=%lld range=[0,%lld)\n",
           w.g->name.c_str(), w.level, w.bx, w.by, w.vx, w.vy, family, what, plane, row, xb, off, (long long)got, (long long)truth, (long long)(got - truth), (long long)range);
}

template <int BPS> struct Audit {
    const Geo &g;
    const Level &L;
    int lvl;
    int nBlkX, nBlkY, pel, logPel, pw, ph, hpad, vpad, chpad, cvpad, stepX, stepY, hps, vps, BW;
    int64_t off0, off1, ps0, ps1, pitch0, pitch1, sh0, sh1;
    bool uv;
    Audit(const Geo &g_, int lvl_) : g(g_), L(g_.lv[lvl_]), lvl(lvl_) {
        nBlkX = (int)L.v[0]; nBlkY = (int)L.v[1]; pel = (int)L.v[2]; logPel = pel == 4 ? 2 : pel == 2 ? 1 : 0;
        pw = (int)L.v[3]; ph = (int)L.v[4]; hpad = (int)L.v[5]; vpad = (int)L.v[6]; chpad = (int)L.v[9]; cvpad = (int)L.v[10];
        off0 = L.v[11]; off1 = L.v[12]; ps0 = L.v[14]; ps1 = L.v[15]; pitch0 = L.v[17]; pitch1 = L.v[18]; sh0 = L.v[20]; sh1 = L.v[21];
        BW = g.blk; stepX = stepY = g.blk - g.ov; hps = hpad >> lvl; vps = vpad >> lvl;
        uv = g.chroma && sh1 != 0;
    }
    void limits(int bx, int by, int &xmin, int &xmax, int &ymin, int &ymax) const { // PlaneOfBlocks.cpp:1094-1097
        const int x0 = hpad + stepX * bx, y0 = vpad + stepY * by;
        xmax = (pw - x0 - BW - hpad + hps) * pel; ymax = (ph - y0 - BW - vpad + vps) * pel; // (<< logPel in the kernels; a negative value shifted left is undefined on the host)
        xmin = -((x0 - hpad + hps) * pel); ymin = -((y0 - vpad + vps) * pel);
    }
    // signed truth: byte position of the luma / chroma block's first sample inside its plane
    int64_t luma_true(int x0, int y0, int vx, int vy) const {
        const int64_t ax = ((int64_t)x0 << logPel) + vx, ay = ((int64_t)y0 << logPel) + vy, m = pel - 1;
        return off0 + ((ax & m) | ((ay & m) << logPel)) * ps0 + (ay >> logPel) * pitch0 + (ax >> logPel) * BPS;
    }
    int64_t chroma_true(int cx0, int cy0, int vx, int vy) const {
        const int64_t ax = ((int64_t)cx0 << logPel) + ((vx + (vx < 0 ? 1 : 0)) >> 1), ay = ((int64_t)cy0 << logPel) + ((vy + (vy < 0 ? 1 : 0)) >> 1), m = pel - 1;
        return off1 + ((ax & m) | ((ay & m) << logPel)) * ps1 + (ay >> logPel) * pitch1 + (ax >> logPel) * BPS;
    }
    int64_t shadow_true(int64_t t) const { // the sample at byte t of the plane, read from the shifted copy it starts a dword in
        if (!sh0) return t;
        const int64_t k = BPS == 2 ? (t >> 1) & 1 : t & 3;
        return (t & ~(int64_t)3) + k * sh0;
    }
    // rows x (rowBytes / cb) pieces from a running offset per piece column
    void block(const Where &w, const char *fam, const char *what, int plane, int64_t base, unsigned off, unsigned pitch, int64_t truth, int rows, int rowBytes, int cb) const {
        for (int xb = 0; xb < rowBytes; xb += cb) {
            unsigned po = mvx_piece_off32(off, 0, pitch, xb);
            for (int r = 0; r < rows; r++) {
                check(w, fam, what, plane, r, xb, base, po, truth + (int64_t)r * pitch + xb, cb);
                po += mvx_rows_step32(1, pitch);
            }
        }
    }
    unsigned luma_off(int x0, int y0, int vx, int vy) const { return mvx_shadow_off<BPS>(mvx_luma_off32<BPS>(x0, y0, vx, vy, pel, logPel, (unsigned)ps0, (unsigned)pitch0), (unsigned)sh0); }
    unsigned chroma_off(int x0, int y0, int vx, int vy) const { return mvx_chroma_off32<BPS>(x0 >> 1, y0 >> 1, vx, vy, 1, 1, pel, logPel, (unsigned)ps1, (unsigned)pitch1); }
    int64_t biasY() const { return mvx_ref_bias_bytes(pitch0, BPS); }
    int64_t biasC() const { return mvx_ref_bias_bytes(pitch1, BPS); }

    // the lean kernel's eval / the speculative kernel's one-block passes (FastSearcher::region, region2; SpecSearcher::pass_start, pass_issue)
    void lean_block(const Where &w, int x0, int y0, int vx, int vy, int vyc) const {
        const int lrow = BW * BPS, lcb = std::min(16, lrow);
        block(w, "lean/spec", "luma", 0, off0 - biasY(), luma_off(x0, y0, vx, vy), (unsigned)pitch0, shadow_true(luma_true(x0, y0, vx, vy)), BW, lrow, lcb);
        if (!g.chroma) return;
        const unsigned co = chroma_off(x0, y0, vx, vyc);
        const int64_t ct = chroma_true(x0 >> 1, y0 >> 1, vx, vyc);
        const int crow = BW / 2 * BPS;
        if (uv) block(w, "lean/spec", "uv", 1, sh1 + 2 * off1 - 2 * biasC(), 2 * co, 2 * (unsigned)pitch1, sh1 + 2 * ct, BW / 2, 2 * crow, std::min(16, 2 * crow));
        else for (int p = 1; p <= 2; p++) block(w, "lean/spec", p == 1 ? "u" : "v", p, off1 - biasC(), co, (unsigned)pitch1, ct, BW / 2, crow, std::min(16, crow));
    }
    // the specialised general kernels (Searcher::eval_fixed, region_fixed32): plain planes, never the copies
    void general_block(const Where &w, int x0, int y0, int cx0, int cy0, int vx, int vy, int vyc) const {
        const int lrow = BW * BPS, crow = BW / 2 * BPS;
        block(w, "general32", "luma", 0, off0 - biasY(), mvx_luma_off32<BPS>(x0, y0, vx, vy, pel, logPel, (unsigned)ps0, (unsigned)pitch0), (unsigned)pitch0, luma_true(x0, y0, vx, vy), BW, lrow, std::min(16, lrow));
        if (!g.chroma) return;
        const unsigned co = mvx_chroma_off32<BPS>(cx0, cy0, vx, vyc, 1, 1, pel, logPel, (unsigned)ps1, (unsigned)pitch1);
        for (int p = 1; p <= 2; p++) block(w, "general32", p == 1 ? "u" : "v", p, off1 - biasC(), co, (unsigned)pitch1, chroma_true(cx0, cy0, vx, vyc), BW / 2, crow, std::min(16, crow));
    }
    // one lane of a row pass: `rowsA` luma rows and, with the UV plane, rowsA / 2 of its rows, `bytes` per load, the block's offsets moved by `extra` bytes
    // (strip_issue / strip8_issue: curA += pitchY, curB += 2 * pitchC)
    void strip_lane(const Where &w, const char *what, int x0, int y0, int vx, int vy, int vyc, int extraA, int extraB, int rowsA, int bytes) const {
        unsigned a = luma_off(x0, y0, vx, vy) + (unsigned)extraA;
        const int64_t ta = shadow_true(luma_true(x0, y0, vx, vy)) + extraA;
        for (int r = 0; r < rowsA; r++) { check(w, "spec-rowpass", what, 0, r, extraA, off0 - biasY(), a, ta + (int64_t)r * pitch0, bytes); a += mvx_rows_step32(1, (unsigned)pitch0); }
        if (!uv) return;
        unsigned b = 2 * chroma_off(x0, y0, vx, vyc) + (unsigned)extraB;
        const int64_t tb = sh1 + 2 * chroma_true(x0 >> 1, y0 >> 1, vx, vyc) + extraB;
        for (int r = 0; r < rowsA / 2; r++) { check(w, "spec-rowpass", what, 1, r, extraB, sh1 + 2 * off1 - 2 * biasC(), b, tb + (int64_t)r * 2 * pitch1, bytes); b += mvx_rows_step32(1, 2 * (unsigned)pitch1); }
    }

    // vectors the reference can load for a block with these limits: clipped predictors (legal or not), the rectangle's extremes, zero
    static void vectors(int xmin, int xmax, int ymin, int ymax, std::vector<std::pair<int, int>> &out) {
        out.clear();
        out.push_back({0, 0});
        auto cx = [&](int v) { return std::min(std::max(v, xmin), xmax - 1); };
        auto cy = [&](int v) { return std::min(std::max(v, ymin), ymax - 1); };
        const int far[3] = { -100000, 0, 100000 };
        for (int a : far) for (int b : far) out.push_back({cx(a), cy(b)});
        if (xmax > xmin && ymax > ymin) {
            const int xs[3] = { xmin, (xmin + xmax - 1) / 2, xmax - 1 }, ys[3] = { ymin, (ymin + ymax - 1) / 2, ymax - 1 };
            for (int a : xs) for (int b : ys) out.push_back({a, b});
        }
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
    }

    void run() const {
        int emptyx = 0, emptyy = 0;
        std::vector<std::pair<int, int>> vs;
        const bool side = g.ov == 0;
        const bool strip16 = g.route == 2 && BW == 16 && (g.ov == 8 || g.ov == 0) && (g.chroma ? uv : true);
        const bool strip8 = g.route == 2 && BPS == 1 && BW == 8 && uv && (g.ov == 4 || g.ov == 0);
        for (int by = 0; by < nBlkY; by++)
            for (int bx = 0; bx < nBlkX; bx++) {
                int xmin, xmax, ymin, ymax;
                limits(bx, by, xmin, xmax, ymin, ymax);
                emptyx += xmax <= xmin; emptyy += ymax <= ymin;
                const int x0 = hpad + stepX * bx, y0 = vpad + stepY * by, cx0 = chpad + (stepX >> 1) * bx, cy0 = cvpad + (stepY >> 1) * by;
                vectors(xmin, xmax, ymin, ymax, vs);
                for (auto &v : vs) {
                    const Where w = { &g, lvl, bx, by, v.first, v.second };
                    if (g.route == 2) lean_block(w, x0, y0, v.first, v.second, v.second); // (the zero candidate's chroma ignores the field shift: no field shift here)
                    if (g.route >= 1) general_block(w, x0, y0, cx0, cy0, v.first, v.second, v.second);
                    if (strip16) { // block lanes of a 16x16 row pass: two lanes per block, COLB bytes each
                        const int colb = BPS == 2 ? 16 : 8;
                        for (int hB = 0; hB < 2; hB++) strip_lane(w, "block-lane", x0, y0, v.first, v.second, v.second, hB * colb, hB * colb, BW, colb);
                    }
                    if (strip8) { // block lanes of the 8-bit 8x8 row pass: sixteen bytes from the block's first sample, eight earlier where that would cross the row's end
                        const int xl = ((x0 << logPel) + v.first) >> logPel, xc = 2 * ((((x0 >> 1) << logPel) + ((v.first + (v.first < 0 ? 1 : 0)) >> 1)) >> logPel);
                        const int shA = xl + 16 > pw ? 2 : 0, shB = xc + 16 > pw ? 2 : 0;
                        strip_lane(w, "block-lane8", x0, y0, v.first, v.second, v.second, -shA * 4, -shB * 4, 8, 16);
                    }
                }
                // strip lanes: one vector for a whole window of blocks that starts here -- the zero vector, and the extremes of what is legal for every block of the window
                if (strip16 || strip8) {
                    const int wblk = strip8 ? (side ? 8 : 15) : (side ? 4 : 7);
                    for (int Lw = 1; Lw <= std::min(wblk, nBlkX - bx); Lw++) { // (the kernel cuts a group of a row into windows of equal length: any start, any length up to a full window)
                    int x2min, x2max, y2min, y2max;
                    limits(bx + Lw - 1, by, x2min, x2max, y2min, y2max);
                    vectors(std::max(xmin, x2min), std::min(xmax, x2max), ymin, ymax, vs);
                    for (auto &v : vs) {
                        const bool zero = v.first == 0 && v.second == 0;
                        // What the kernel never forms is left out: the 8-bit 8x8 row passes have no window of fewer than four dwords (rows8: "a window has at
                        // least four dwords", groups of one or two blocks go one block at a time -- lean_block above), and stage 2 runs no window of one block as a strip.
                        if (strip8 && (side ? 2 * Lw : Lw + 1) < 4) continue;
                        if (!zero && Lw < 2) continue;
                        if (!zero && !(v.first >= std::max(xmin, x2min) && v.first < std::min(xmax, x2max) && v.second >= ymin && v.second < ymax)) continue; // (stage 2 runs a window as a strip only with the whole pattern legal)
                        const Where w = { &g, lvl, bx, by, v.first, v.second };
                        if (strip16) {
                            const int colb = BPS == 2 ? 16 : 8, tc = side ? 2 : 1;
                            for (int p = 0; p < 8; p++) {
                                const int pe = std::min(p, tc * (Lw - 1) + 1) * colb; // (columns beyond the run re-read its last one)
                                strip_lane(w, "strip-lane", x0, y0, v.first, v.second, v.second, pe, pe, BW, colb);
                            }
                        } else {
                            const int nd = side ? 2 * Lw : Lw + 1; // the window's dwords
                            for (int qS = 0; qS < 4; qS++) {
                                const int qe = std::min(qS, (nd - 1) >> 2), d0 = std::min(4 * qe, nd - 4); // (the lane with the window's last dwords starts early enough to end with them)
                                strip_lane(w, "strip-lane8", x0, y0, v.first, v.second, v.second, d0 * 4, d0 * 4, 8, 16);
                            }
                        }
                    }
                    }
                }
            }
        printf("level %s %d emptyx=%d emptyy=%d blocks=%d\n", g.name.c_str(), lvl, emptyx, emptyy, nBlkX * nBlkY);
    }
};

int main() {
    std::vector<Geo> geos;
    char key[8], name[256];
    while (scanf("%7s", key) == 1) {
        if (!strcmp(key, "G")) {
            Geo g;
            int nl;
            long long r0, r1;
            if (scanf("%255s %d %d %d %d %d %lld %lld %d", name, &g.bps, &g.chroma, &g.blk, &g.ov, &g.route, &r0, &r1, &nl) != 9) { fprintf(stderr, "bad G line\n"); return 2; }
            if ((g.bps != 1 && g.bps != 2) || nl < 1 || nl > 32 || g.blk < 4 || g.ov < 0 || g.ov > g.blk / 2) { fprintf(stderr, "bad geometry\n"); return 2; }
            g.name = name; g.range[0] = r0; g.range[1] = r1;
            geos.push_back(g);
        } else if (!strcmp(key, "L") && !geos.empty()) {
            Level l;
            for (int i = 0; i < 24; i++) { long long t; if (scanf("%lld", &t) != 1) { fprintf(stderr, "bad L line\n"); return 2; } l.v[i] = t; }
            if (l.v[2] != 1 && l.v[2] != 2 && l.v[2] != 4) { fprintf(stderr, "bad pel\n"); return 2; }
            geos.back().lv.push_back(l);
        } else { fprintf(stderr, "bad input\n"); return 2; }
    }
    int bad = 0;
    for (const Geo &g : geos) {
        g_accesses = 0; g_bad = false;
        if (g.route == 0) { printf("generic %s (64-bit addresses: nothing to audit)\n", g.name.c_str()); continue; }
        for (int l = 0; l < (int)g.lv.size(); l++) {
            if (g.bps == 1) Audit<1>(g, l).run(); else Audit<2>(g, l).run();
        }
        if (g_bad) bad++; else printf("ok %s accesses=%lld\n", g.name.c_str(), g_accesses);
    }
    printf("search_addressing_host_main: %d of %d geometries with a violation\n", bad, (int)geos.size());
    return bad ? 1 : 0;
}
