/* The oracle at the ends of the sample range, as a stand-alone program for AddressSanitizer / UndefinedBehaviourSanitizer
 * (tests/test_sample_range.py builds and runs it; any report aborts, a clean run exits 0).
 *
 * It makes the `step` and `checker` clips of tests/sample_range.py itself -- same arithmetic, same LCG; the checksums it prints are
 * compared with the Python generators' -- at 16 and at 10 bits, 256x160 4:2:0, three frames, and runs
 *   Super -> Analyse (blksize 32 / overlap 16 and 16 / 8, pnew 50 and 256, both directions) -> Degrain1 (with and without limits) -> Compensate
 * through the oracle's C functions.  At 16 bits the step is 0 -> 49152: pnew * SAD passes 2^31 for every combination.
 * TEST INFRASTRUCTURE ONLY. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mvoracle.h"

enum { W = 256, H = 160, NF = 3 };

typedef struct { uint8_t *p[3]; int pitch[3]; int w[3], h[3]; } frame_t;

static uint32_t lcg_state;
static unsigned lcg_next(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 16; }

static frame_t frame_alloc(int w, int h, int bps) {
    frame_t f;
    for (int p = 0; p < 3; p++) {
        f.w[p] = p ? w / 2 : w; f.h[p] = p ? h / 2 : h;
        f.pitch[p] = f.w[p] * bps;
        f.p[p] = (uint8_t *)calloc((size_t)f.pitch[p] * f.h[p], 1);
        if (!f.p[p]) exit(2);
    }
    return f;
}
static void frame_free(frame_t *f) { for (int p = 0; p < 3; p++) free(f->p[p]); }
static void put(frame_t *f, int p, int x, int y, int bps, int v) {
    if (bps == 1) f->p[p][y * f->pitch[p] + x] = (uint8_t)v; else ((uint16_t *)(f->p[p] + (size_t)y * f->pitch[p]))[x] = (uint16_t)v;
}
static int get(const frame_t *f, int p, int x, int y, int bps) {
    return bps == 1 ? f->p[p][y * f->pitch[p] + x] : ((const uint16_t *)(f->p[p] + (size_t)y * f->pitch[p]))[x];
}

/* sample_range.step: even frames lo + n, odd frames hi - n, n = (r * (amp + 1)) >> 16, amp = 2^bits / 32 */
static void make_step(frame_t *fr, int bits, int lo, int hi) {
    const int bps = bits > 8 ? 2 : 1, amp = (1 << bits) / 32;
    lcg_state = 12345;
    for (int f = 0; f < NF; f++) {
        fr[f] = frame_alloc(W, H, bps);
        for (int p = 0; p < 3; p++)
            for (int y = 0; y < fr[f].h[p]; y++)
                for (int x = 0; x < fr[f].w[p]; x++) {
                    const int n = (int)((lcg_next() * (unsigned)(amp + 1)) >> 16);
                    put(&fr[f], p, x, y, bps, (f & 1) ? hi - n : lo + n);
                }
    }
}

/* sample_range.checker: 3x3 cells of 0 and pm in every plane's own grid, moving by (2, 1) per frame */
static void make_checker(frame_t *fr, int bits) {
    const int bps = bits > 8 ? 2 : 1, pm = (1 << bits) - 1, cell = 3;
    for (int f = 0; f < NF; f++) {
        fr[f] = frame_alloc(W, H, bps);
        for (int p = 0; p < 3; p++)
            for (int y = 0; y < fr[f].h[p]; y++)
                for (int x = 0; x < fr[f].w[p]; x++) {
                    const int xs = x - 2 * f + 3 * cell * NF, ys = y - f + 3 * cell * NF;
                    put(&fr[f], p, x, y, bps, pm * ((xs / cell + ys / cell) & 1));
                }
    }
}

static long long checksum(const frame_t *fr, int bps) {
    long long s = 0;
    for (int f = 0; f < NF; f++)
        for (int p = 0; p < 3; p++) {
            long long t = 0;
            for (int y = 0; y < fr[f].h[p]; y++)
                for (int x = 0; x < fr[f].w[p]; x++) t += get(&fr[f], p, x, y, bps);
            s += t * (7 * f + p + 1);
        }
    return s;
}

static void die(const char *what, const char *err) { fprintf(stderr, "%s: %s\n", what, err); exit(3); }

static void run_clip(const char *name, frame_t *fr, int bits) {
    char err[MVO_ERR];
    const int bps = bits > 8 ? 2 : 1, pm = (1 << bits) - 1;
    printf("clip %s %lld\n", name, checksum(fr, bps));
    mvo_super s;
    if (mvo_super_init(&s, W, H, bits, 1, 1, 0, MVO_UNSET, MVO_UNSET, MVO_UNSET, MVO_UNSET, MVO_UNSET, MVO_UNSET, MVO_UNSET, err)) die("super", err);
    frame_t sup[NF];
    for (int f = 0; f < NF; f++) {
        sup[f] = frame_alloc(s.superWidth, s.superHeight, bps);
        mvo_super_frame(&s, (const uint8_t *const *)fr[f].p, fr[f].pitch, sup[f].p, sup[f].pitch);
    }
    static const int shapes[2][2] = { { 32, 16 }, { 16, 8 } };
    static const int pnews[2] = { 50, 256 };
    for (int sh = 0; sh < 2; sh++)
        for (int pn = 0; pn < 2; pn++) {
            mvo_analyse an[2];
            uint8_t *blob[2];
            for (int isb = 1; isb >= 0; isb--) { /* order of Degrain's references: backward, forward */
                mvo_analyse_args a;
                mvo_analyse_args_default(&a);
                a.blksize = shapes[sh][0]; a.overlap = shapes[sh][1]; a.pnew = pnews[pn]; a.isb = isb;
                mvo_analyse *d = &an[1 - isb];
                if (mvo_analyse_init(d, &a, &s, NF, err)) die("analyse", err);
                blob[1 - isb] = (uint8_t *)calloc((size_t)mvo_analyse_blob_size(d), 1);
                const frame_t *ref = &sup[isb ? 2 : 0];
                mvo_analyse_frame(d, (const uint8_t *const *)sup[1].p, sup[1].pitch, (const uint8_t *const *)ref->p, ref->pitch, 0, blob[1 - isb]);
            }
            const mvo_vector *v = mvo_blob_level0(&an[0].ad, blob[0]);
            long long sad = 0;
            for (int i = 0; i < an[0].ad.nBlkX * an[0].ad.nBlkY; i++) sad += v[i].sad;
            printf("  blk %d pnew %d: level-0 SAD sum %lld\n", shapes[sh][0], pnews[pn], sad);
            for (int lim = 0; lim < 2; lim++) {
                mvo_degrain dg;
                if (mvo_degrain_init(&dg, 1, &an[0].ad, &s, MVO_UNSET, MVO_UNSET, MVO_UNSET, lim ? pm / 100 : MVO_UNSET, lim ? pm / 100 : MVO_UNSET, MVO_UNSET, MVO_UNSET, err))
                    die("degrain", err);
                frame_t out = frame_alloc(W, H, bps);
                const uint8_t *refs[2][3]; int rpitch[2][3];
                for (int r = 0; r < 2; r++)
                    for (int p = 0; p < 3; p++) { refs[r][p] = sup[r ? 0 : 2].p[p]; rpitch[r][p] = sup[r ? 0 : 2].pitch[p]; }
                const uint8_t *bl[2] = { blob[0], blob[1] };
                mvo_degrain_frame(&dg, (const uint8_t *const *)fr[1].p, fr[1].pitch, (const uint8_t *const (*)[3])refs, (const int (*)[3])rpitch, bl, out.p, out.pitch);
                frame_free(&out);
            }
            for (int th = 0; th < 2; th++) {
                mvo_compensate c;
                if (mvo_compensate_init(&c, &an[0].ad, &s, MVO_UNSET, th ? 1 : MVO_UNSET, 100.0, MVO_UNSET, MVO_UNSET, err)) die("compensate", err);
                frame_t out = frame_alloc(W, H, bps);
                mvo_compensate_frame(&c, (const uint8_t *const *)sup[1].p, sup[1].pitch, (const uint8_t *const *)sup[2].p, sup[2].pitch, blob[0], out.p, out.pitch, 0);
                frame_free(&out);
            }
            free(blob[0]); free(blob[1]);
        }
    for (int f = 0; f < NF; f++) { frame_free(&sup[f]); frame_free(&fr[f]); }
}

int main(void) {
    static const int depths[2] = { 16, 10 };
    for (int i = 0; i < 2; i++) {
        const int bits = depths[i], pm = (1 << bits) - 1;
        frame_t fr[NF];
        char name[32];
        make_step(fr, bits, 0, pm - pm / 4);
        snprintf(name, sizeof name, "step%d", bits);
        run_clip(name, fr, bits);
        make_checker(fr, bits);
        snprintf(name, sizeof name, "checker%d", bits);
        run_clip(name, fr, bits);
    }
    return 0;
}
