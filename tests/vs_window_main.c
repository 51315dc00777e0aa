/* The window arithmetic of the VapourSynth shell (vsplugin/mvx_vs_window.h) on its own: no device, no host.  tests/test_vs_window_host.py compiles this with
 * -fsanitize=address,undefined and runs it; every expectation below is worked out by hand from the definitions in DESIGN.md 4.3.2. */
#include <stdio.h>
#include <stdlib.h>

#include "mvx_vs_window.h"

static int g_failed;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed = 1; } } while (0)

static void check_inputs(int v, int B, int numFrames, int before, int after, int first, int count, int lo, int hi) {
    int f = -1, c = -1, l = -1, h = -1;
    mvx_win_inputs(v, B, numFrames, before, after, &f, &c, &l, &h);
    if (f != first || c != count || l != lo || h != hi) {
        printf("FAILED window %d of %d frames, B %d, -%d +%d: frames %d+%d inputs %d..%d, expected %d+%d %d..%d\n", v, numFrames, B, before, after, f, c, l, h, first, count, lo, hi);
        g_failed = 1;
    }
}

int main(void) {
    /* ---- the default length: 768 chains / (2 * radius) per frame, at least 8, at most mv.Analyse's length */
    CHECK(mvx_win_default_length(1, 128) == 128);  /* 384 */
    CHECK(mvx_win_default_length(3, 128) == 128);  /* 128: the Degrain3 graph itself */
    CHECK(mvx_win_default_length(8, 128) == 48);
    CHECK(mvx_win_default_length(24, 128) == 16);
    CHECK(mvx_win_default_length(1, 16) == 16);
    CHECK(mvx_win_default_length(3, 16) == 16);
    CHECK(mvx_win_default_length(8, 16) == 16);    /* 48 */
    CHECK(mvx_win_default_length(24, 16) == 16);
    CHECK(mvx_win_default_length(24, 4) == 4);     /* a length below the minimum wins: the user asked for it */
    CHECK(mvx_win_default_length(3, 0) == 0);      /* look-ahead off */

    /* ---- input ranges: 11 frames at radius 2 */
    check_inputs(0, 4, 11, 2, 2, 0, 4, 0, 5);      /* the clip's start cuts the frames before */
    check_inputs(1, 4, 11, 2, 2, 4, 4, 2, 9);
    check_inputs(2, 4, 11, 2, 2, 8, 3, 6, 10);     /* the clip end inside the window: 3 frames, nothing behind them */
    check_inputs(2, 5, 11, 2, 2, 10, 1, 8, 10);    /* a last window of one frame */
    check_inputs(0, 128, 11, 2, 2, 0, 11, 0, 10);  /* one window holds the clip */
    check_inputs(0, 1, 11, 2, 2, 0, 1, 0, 2);
    check_inputs(10, 1, 11, 2, 2, 10, 1, 8, 10);
    /* the radius exceeds the window: 17 frames at radius 7, windows of 4 */
    check_inputs(0, 4, 17, 7, 7, 0, 4, 0, 10);
    check_inputs(1, 4, 17, 7, 7, 4, 4, 0, 14);
    check_inputs(2, 4, 17, 7, 7, 8, 4, 1, 16);
    check_inputs(4, 4, 17, 7, 7, 16, 1, 9, 16);
    /* mv.Analyse's shapes: backward delta 1 needs one frame behind, forward delta 2 two frames before */
    check_inputs(1, 8, 37, 0, 1, 8, 8, 8, 16);
    check_inputs(4, 8, 37, 0, 1, 32, 5, 32, 36);
    check_inputs(1, 8, 37, 2, 0, 8, 8, 6, 15);
    check_inputs(0, 8, 37, 2, 0, 0, 8, 0, 7);

    /* ---- the field-to-frame map: mvbw1, mvfw1, mvbw2, mvfw2, ... */
    CHECK(mvx_win_field_offset(0) == 1 && mvx_win_field_offset(1) == -1 && mvx_win_field_offset(2) == 2 && mvx_win_field_offset(3) == -2);
    CHECK(mvx_win_field_offset(46) == 24 && mvx_win_field_offset(47) == -24);
    CHECK(mvx_win_field_input(0, 0, 0, 5) == 1);   /* frame 1 is input 1 of window 0 */
    CHECK(mvx_win_field_input(0, 1, 0, 5) == -1);  /* frame -1: outside the clip */
    CHECK(mvx_win_field_input(3, 2, 0, 5) == 5);   /* the last input of window 0 */
    CHECK(mvx_win_field_input(10, 0, 6, 10) == -1);/* frame 11 of 11 */
    CHECK(mvx_win_field_input(10, 3, 6, 10) == 2);
    CHECK(mvx_win_field_input(8, 3, 6, 10) == 0);
    /* every reference of every frame of every window lies in the window's inputs exactly when it lies in the clip */
    for (int B = 1; B <= 6; B++)
        for (int radius = 1; radius <= 7; radius++)
            for (int numFrames = 2; numFrames <= 17; numFrames += 5)
                for (int n = 0; n < numFrames; n++) {
                    int first, count, lo, hi;
                    mvx_win_inputs(mvx_win_of(n, B), B, numFrames, radius, radius, &first, &count, &lo, &hi);
                    CHECK(n >= first && n < first + count && lo >= 0 && hi < numFrames);
                    for (int r = 0; r < 2 * radius; r++) {
                        const int m = n + mvx_win_field_offset(r), in = m >= 0 && m < numFrames;
                        CHECK(mvx_win_field_input(n, r, lo, hi) == (in ? m - lo : -1));
                    }
                }

    /* ---- slots */
    CHECK(mvx_win_of(0, 4) == 0 && mvx_win_of(3, 4) == 0 && mvx_win_of(4, 4) == 1 && mvx_win_of(9, 4) == 2 && mvx_win_of(10, 128) == 0);
    CHECK(mvx_win_slot(0, 6) == 0 && mvx_win_slot(5, 6) == 5 && mvx_win_slot(6, 6) == 0 && mvx_win_slot(7, 6) == 1);  /* window 6 recycles window 0's slot */

    /* ---- the budget: 3 windows pin 128 + 6 super frames of 1.2, six slots keep 128 blobs of 0.5 */
    CHECK(mvx_win_bytes(128, 2, 6, 1.2, 0.5, 6) > 866.3 && mvx_win_bytes(128, 2, 6, 1.2, 0.5, 6) < 866.5);
    { int B = 128, depth = 2; CHECK(mvx_win_fit(&B, &depth, 6, 1.2, 0.5, 6, 900.0) == 1 && B == 128 && depth == 2); }
    { int B = 128, depth = 2; CHECK(mvx_win_fit(&B, &depth, 6, 1.2, 0.5, 6, 800.0) == 1 && B == 128 && depth == 1); }   /* 705.6: the depth goes first */
    { int B = 128, depth = 2; CHECK(mvx_win_fit(&B, &depth, 6, 1.2, 0.5, 6, 500.0) == 1 && B == 64 && depth == 0); }    /* 544.8 at depth 0, then 276 at 64 frames */
    { int B = 128, depth = 2; CHECK(mvx_win_fit(&B, &depth, 6, 1.2, 0.5, 6, 41.0) == 1 && B == 8 && depth == 0); }     /* 14 * 1.2 + 48 * 0.5 = 40.8 */
    { int B = 128, depth = 2; CHECK(mvx_win_fit(&B, &depth, 6, 1.2, 0.5, 6, 40.0) == 0 && B == 8 && depth == 0); }     /* not even a window of 8: the per-frame path */
    { int B = 4, depth = 3; CHECK(mvx_win_fit(&B, &depth, 4, 1.0, 1.0, 6, 1e9) == 1 && B == 4 && depth == 3); }         /* a short window that fits stays */
    { int B = 4, depth = 1; CHECK(mvx_win_fit(&B, &depth, 4, 1.0, 1.0, 6, 30.0) == 0 && B == 4 && depth == 0); }        /* ... and is not shortened: 8 + 24 */
    /* mv.Analyse's form: (depth + 1) * (B + delta) * (super frame + blob), no slot term */
    CHECK(mvx_win_bytes(128, 2, 1, 10.0, 0.0, 0) == 3870.0);
    { int B = 128, depth = 2; CHECK(mvx_win_fit(&B, &depth, 1, 10.0, 0.0, 0, 1000.0) == 1 && B == 64 && depth == 0); }  /* 1290 at depth 0, 650 at 64 */

    if (g_failed) return 1;
    printf("OK\n");
    return 0;
}
