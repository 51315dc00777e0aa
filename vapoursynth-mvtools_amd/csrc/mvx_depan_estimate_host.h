// mvx_depan_estimate_host.h -- the host side of DepanEstimate, plain C++ without HIP: the creation rules (depanEstimateCreate,
// MVDepan.cpp:1271-1433), everything of get_motion_vector after its scan (:769-882), the combination of the two windows into a zoom
// (:1083-1121), the frame-0 rule (:1137-1140) and stage 3 (:1200-1212).  All of it in float, in the reference's order.  mvx_depan_fft.hip
// includes it; tests/depan_estimate_host_main.cpp runs it as a stand-alone program under the sanitizers.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct DepanEstimateParams {
    float trust_limit, zoommax, stab, pixaspect;
    int winx, winy, wleft, wtop, dxmax, dymax;
    int fields, tff, tff_exists;
    int width, height, bits, num_frames;
    int nwin;               // 1, or 2 with zoommax != 1
};

struct DepanEstimateScan { float max, sum; int imax, jmax; float xp, xm, yp, ym; };
struct DepanEstimateResult { float dx, dy, zoom, trust; };

static inline bool depan_estimate_pow2(int v) { return v >= 8 && v <= 8192 && (v & (v - 1)) == 0; }

// the largest power of two that fits, up to 8192 (:1372-1377)
static inline int depan_estimate_auto_window(int room) {
    int w = 1;
    for (int i = 0; i < 13; i++) if (w * 2 <= room) w = w * 2;
    return w;
}

// returns NULL, or the message of the first failed check.  winx / winy 0 and wleft / wtop / dxmax / dymax < 0 mean "not passed".
static inline const char *depan_estimate_resolve(DepanEstimateParams *P, bool float_samples) {
    if (P->trust_limit < 0.0f || P->trust_limit > 100.0f) return "DepanEstimate: trust must be between 0.0 and 100.0 (inclusive).";
    if (P->pixaspect <= 0.0f) return "DepanEstimate: pixaspect must be positive.";
    if ((!float_samples && (P->bits > 16 || P->bits < 8)) || (float_samples && P->bits != 32))
        return "DepanEstimate: clip must have constant format and dimensions, it must be YUV or Gray, and it must be 8..16 bit integer or 32 bit float.";
    const int wleft0 = P->wleft;
    if (P->wleft < 0) P->wleft = 0;
    if (P->winx > P->width - P->wleft) return "DepanEstimate: winx must not be greater than width-wleft.";
    if (P->winx == 0) P->winx = depan_estimate_auto_window(P->width - P->wleft);
    P->nwin = P->zoommax != 1.0f ? 2 : 1;
    if (P->zoommax != 1.0f) {
        P->winx = P->winx / 2;
        if (wleft0 < 0) P->wleft = (P->width - P->winx * 2) / 4;
    } else if (wleft0 < 0)
        P->wleft = (P->width - P->winx) / 2;
    const int wtop0 = P->wtop;
    if (P->wtop < 0) P->wtop = 0;
    if (P->winy > P->height - P->wtop) return "DepanEstimate: winy must not be greater than height-wtop.";
    if (P->winy == 0) P->winy = depan_estimate_auto_window(P->height - P->wtop);
    if (wtop0 < 0) P->wtop = (P->height - P->winy) / 2;
    if (P->dxmax < 0) P->dxmax = P->winx / 4;
    if (P->dymax < 0) P->dymax = P->winy / 4;
    if (P->dxmax >= P->winx / 2) return "DepanEstimate: dxmax must be less than winx/2.";
    if (P->dymax >= P->winy / 2) return "DepanEstimate: dymax must be less than winy/2.";
    // the library's own refusals (divergences 8 to 10 of mvtools_amd.h)
    if (float_samples) return "DepanEstimate: float clips are not supported.";
    if (!depan_estimate_pow2(P->winx) || !depan_estimate_pow2(P->winy))
        return "DepanEstimate: winx (after the halving for zoom) and winy must be powers of two between 8 and 8192.";
    if (P->wleft + (P->nwin == 2 ? P->width / 2 : 0) + P->winx > P->width || P->wtop + P->winy > P->height)
        return "DepanEstimate: every window must lie inside the frame.";
    return NULL;
}

// get_motion_vector from `trust` on, MVDepan.cpp:769-882, on what the scan of the surface left
static inline void depan_estimate_vector(const DepanEstimateParams &P, const DepanEstimateScan &S, int top_field, float *fdx, float *fdy, float *trust) {
    const int winx = P.winx, winy = P.winy, dxmax = P.dxmax, dymax = P.dymax;
    const float stab = P.stab;
    const int count = (2 * dxmax + 1) * (2 * dymax + 1);
    float correlmax = S.max, correlmean = S.sum;
    float xadd = 0.0f, yadd = 0.0f, f1, f2;
    int dx, dy;
    correlmean = correlmean / count;
    correlmax = correlmax / (winx * winy);
    correlmean = correlmean / (winx * winy);
    *trust = (correlmax - correlmean) * 100.0f / (correlmax + 0.1f);
    dx = S.imax * 2 < winx ? S.imax : S.imax - winx;
    dy = S.jmax * 2 < winy ? S.jmax : S.jmax - winy;
    *trust *= (dxmax + 1) / (dxmax + 1 + stab * abs(dx)) * (dymax + 1) / (dymax + 1 + stab * abs(dy));
    if (*trust < P.trust_limit) {
        *fdx = 0.0f;
        *fdy = 0.0f;
        return;
    }
    f1 = (S.xp - S.xm) / 2.0f;
    f2 = S.xp + S.xm - S.max * 2.0f;
    if (f2 == 0.0f)
        xadd = 0.0f;
    else {
        xadd = -f1 / f2;
        if (xadd > 1.0f) xadd = 1.0f;
        else if (xadd < -1.0f) xadd = -1.0f;
    }
    if (fabsf(dx + xadd) > dxmax) xadd = 0.0f;
    f1 = (S.yp - S.ym) / 2.0f;
    f2 = S.yp + S.ym - S.max * 2.0f;
    if (f2 == 0.0f)
        yadd = 0.0f;
    else {
        yadd = -f1 / f2;
        if (yadd > 1.0f) yadd = 1.0f;
        else if (yadd < -1.0f) yadd = -1.0f;
    }
    if (fabsf(dy + yadd) > dymax) yadd = 0.0f;
    if (P.fields) {
        if (top_field) yadd += 0.5f;
        else yadd += -0.5f;
        yadd = yadd * 2.0f;
        dy = dy * 2;
    }
    *fdx = (float)dx + xadd;
    *fdy = (float)dy + yadd;
    *fdy = (*fdy) / P.pixaspect;
    if (fabsf(*fdx) < 0.01f) *fdx = 0.011f; // the reference draws the sign from rand(): divergence 1
}

// stage 2 after the transforms, :1063-1140.  scans: one per window.  top_field: the _Field property, < 0 when absent (read with fields only).
// Returns false when fields is set and neither the property nor tff is there.
static inline bool depan_estimate_pair(const DepanEstimateParams &P, const DepanEstimateScan *scans, int top_field, int n, DepanEstimateResult *out) {
    int top = 0;
    if (P.fields) {
        if (top_field < 0 && !P.tff_exists) return false;
        top = top_field < 0 ? 0 : !!top_field;
        if (P.tff_exists) top = P.tff ^ (n % 2);
    }
    float dx1, dy1, trust1;
    depan_estimate_vector(P, scans[0], top, &dx1, &dy1, &trust1);
    float motionx, motiony, motionzoom, trust;
    if (P.nwin == 1) {
        motionzoom = 1.0f;
        motionx = dx1;
        motiony = dy1;
        trust = trust1;
    } else {
        float dx2, dy2, trust2;
        depan_estimate_vector(P, scans[1], top, &dx2, &dy2, &trust2);
        const int winleft = P.wleft, winleft2 = P.wleft + P.width / 2;
        const float zoom = 1.0f + (dx2 - dx1) / (winleft2 - winleft);
        if ((dx1 != 0.0f) && (dx2 != 0.0f) && (fabsf(zoom - 1.0f) < (P.zoommax - 1.0f))) {
            motionx = (dx1 + dx2) / 2.0f;
            motiony = (dy1 + dy2) / 2.0f;
            motionzoom = zoom;
        } else {
            motionx = 0.0f;
            motiony = 0.0f;
            motionzoom = 1.0f;
        }
        trust = trust1 < trust2 ? trust1 : trust2;
    }
    if (n == 0) {
        motionx = motiony = trust = 0.0f;
        motionzoom = 1.0f;
    }
    out->dx = motionx; out->dy = motiony; out->zoom = motionzoom; out->trust = trust;
    return true;
}

// stage 3, :1200-1212: r[0], r[1], r[2] are the results of frames max(0, n - 1), n, min(n + 1, num_frames - 1); motion = dx, dy, zoom, rot
static inline void depan_estimate_finish(const DepanEstimateParams &P, int n, const DepanEstimateResult r[3], float motion[4]) {
    float motionx = r[1].dx, motiony = r[1].dy, motionzoom = r[1].zoom;
    const float t0 = r[0].trust, t1 = r[1].trust, t2 = r[2].trust;
    if (n - 1 >= 0 && n < P.num_frames && t1 < P.trust_limit * 2.0f && t1 < 0.5f * t0) {
        motionx = 0.0f; motiony = 0.0f; motionzoom = 1.0f;
    }
    if (n >= 0 && n + 1 < P.num_frames && t1 < P.trust_limit * 2.0f && t1 < 0.5f * t2) {
        motionx = 0.0f; motiony = 0.0f; motionzoom = 1.0f;
    }
    motion[0] = motionx; motion[1] = motiony; motion[2] = motionzoom; motion[3] = 0.0f;
}
