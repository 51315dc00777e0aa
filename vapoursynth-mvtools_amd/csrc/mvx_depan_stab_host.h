// mvx_depan_stab_host.h -- the host arithmetic of DepanStabilise, without HIP so that a stand-alone program can include it: the creation
// constants (MVDepan.cpp:4059-4163), Inertial (:2945-3115), Average (:3118-3246), InertialLimit (:3249-3329), the two drivers
// (depanStabiliseGetFrame0 :3562-3666, depanStabiliseGetFrame1 :3712-3841) and the source selection of fillBorderPrev (:3395-3422) and
// fillBorderNext (:3458-3505).  It builds on the transform algebra of mvx_depan_host.h.  Every expression is the reference's, in its order,
// in float: build with -ffp-contract=off.  The reference is C++ and includes <math.h>, so sqrt / fabs / isfinite of a float are the float
// overloads there as here (the static_assert below); `1 + sqrt(...)` of InertialLimit's zoom limit is therefore a float sum.
#pragma once
#include <limits.h>
#include "mvx_depan_host.h"

static_assert(sizeof(sqrt(1.0f)) == sizeof(float) && sizeof(fabs(1.0f)) == sizeof(float), "sqrt(float) and fabs(float) must be the float overloads, as in the reference");

struct DepanStabParams {
    // arguments, rounded to float as the reference stores them; initzoom and zoommax as creation leaves them (:4061, :4138)
    float cutoff, damping, initzoom, dxmax, dymax, zoommax, rotmax, pixaspect, tzoom;
    int addzoom, prev, next, mirror, blur, subpixel, fitlast, method, fields;
    int width, height, num_frames;
    // derived
    int nfields, radius, wintsize, winrzsize, winfzsize;
    float fps, freqnative, xcenter, ycenter;
    DepanTransform nonlinfactor;
    std::vector<float> wint, winrz, winfz;
};

// (int) of a float the way the reference writes it, but defined for every value: saturating, NaN -> 0
static inline int depan_stab_to_int(float v) {
    if (!(v == v)) return 0;
    if (v >= 2147483648.0f) return INT_MAX;
    if (v <= -2147483648.0f) return INT_MIN;
    return (int)v;
}

// MVDepan.cpp:4059-4163.  The arguments, width, height and num_frames are set; initzoom and zoommax as passed.
static inline void depan_stab_init(DepanStabParams *d, long long fps_num, long long fps_den) {
    float lambda;
    d->zoommax = d->zoommax > 0 ? (d->zoommax > d->initzoom ? d->zoommax : d->initzoom) : -(-d->zoommax > d->initzoom ? -d->zoommax : d->initzoom);
    d->nfields = d->fields ? 2 : 1;
    lambda = sqrtf(1 + 6 * d->damping * d->damping + sqrtf((1 + 6 * d->damping * d->damping) * (1 + 6 * d->damping * d->damping) + 3));
    d->freqnative = d->cutoff / lambda;
    d->fps = (float)fps_num / fps_den;
    if (d->dxmax != 0.0f) d->nonlinfactor.dxc = 5 / fabsf(d->dxmax); else d->nonlinfactor.dxc = 0;
    if (fabsf(d->zoommax) != 1.0f) { d->nonlinfactor.dxx = 5 / (fabsf(d->zoommax) - 1); d->nonlinfactor.dyy = 5 / (fabsf(d->zoommax) - 1); }
    else { d->nonlinfactor.dxx = 0; d->nonlinfactor.dyy = 0; }
    if (d->dymax != 0.0f) d->nonlinfactor.dyc = 5 / fabsf(d->dymax); else d->nonlinfactor.dyc = 0;
    if (d->rotmax != 0.0f) { d->nonlinfactor.dxy = 5 / fabsf(d->rotmax); d->nonlinfactor.dyx = 5 / fabsf(d->rotmax); }
    else { d->nonlinfactor.dxy = 0; d->nonlinfactor.dyx = 0; }
    d->initzoom = 1 / d->initzoom;
    d->wintsize = depan_stab_to_int(d->fps / (4 * d->cutoff));
    d->radius = d->wintsize;
    d->wint.assign((size_t)d->wintsize + 1, 0.0f);
    float PI = 3.14159265258f;
    for (int i = 0; i < d->wintsize; i++) d->wint[i] = cosf(i * 0.5f * PI / d->wintsize);
    d->wint[d->wintsize] = 0;
    d->winrz.assign((size_t)d->wintsize + 1, 0.0f);
    d->winfz.assign((size_t)d->wintsize + 1, 0.0f);
    const int tz = depan_stab_to_int(d->fps * d->tzoom / 4);
    d->winrzsize = d->wintsize < tz ? d->wintsize : tz;
    d->winfzsize = d->wintsize < tz ? d->wintsize : tz;
    for (int i = 0; i < d->winrzsize; i++) d->winrz[i] = cosf(i * 0.5f * PI / d->winrzsize);
    for (int i = d->winrzsize; i <= d->wintsize; i++) d->winrz[i] = 0;
    for (int i = 0; i < d->winfzsize; i++) d->winfz[i] = cosf(i * 0.5f * PI / d->winfzsize);
    for (int i = d->winfzsize; i <= d->wintsize; i++) d->winfz[i] = 0;
    d->xcenter = d->width / 2.0f;
    d->ycenter = d->height / 2.0f;
}

// an array indexed by frame number from `first` on, as the reference's `trcumul - nbase`, without forming a pointer outside the array
template <typename T> struct DepanStabFrom {
    T *p; int first;
    T &operator[](int n) const { return p[n - first]; }
};

// the motion of data frame n as the filter holds it: frame 0 is set at creation and never read from the data clip (:4075-4078).
// m: dx, dy, zoom, rot of data frames first, first + 1, ...
struct DepanStabMotions {
    const float *m; int first;
    float x(int n) const { return n == 0 ? 0.0f : m[4 * (n - first)]; }
    float y(int n) const { return n == 0 ? 0.0f : m[4 * (n - first) + 1]; }
    float zoom(int n) const { return n == 0 ? 1.0f : m[4 * (n - first) + 2]; }
    float rot(int n) const { return n == 0 ? 0.0f : m[4 * (n - first) + 3]; }
};

static inline void depan_stab_frame_transform(const DepanStabParams *d, const DepanStabMotions &M, int n, DepanTransform *tr) {
    depan_motion2transform(M.x(n), M.y(n), M.rot(n), M.zoom(n), d->pixaspect / d->nfields, d->xcenter, d->ycenter, 1, 1.0f, tr);
}

// the adaptive zoom factor of :3040-3052 / :3191-3203
static inline float depan_stab_azoom(const DepanStabParams *d, const DepanTransform &trcur) {
    const float xcenter = d->xcenter, ycenter = d->ycenter;
    const int width = d->width, height = d->height;
    float azoom = d->initzoom;
    float azoomtest = 1 + (trcur.dxc + trcur.dxy * ycenter) / xcenter; // xleft
    if (azoomtest < azoom) azoom = azoomtest;
    azoomtest = 1 - (trcur.dxc + trcur.dxx * width + trcur.dxy * ycenter - width) / xcenter; // xright
    if (azoomtest < azoom) azoom = azoomtest;
    azoomtest = 1 + (trcur.dyc + trcur.dyx * xcenter) / ycenter; // ytop
    if (azoomtest < azoom) azoom = azoomtest;
    azoomtest = 1 - (trcur.dyc + trcur.dyx * xcenter + trcur.dyy * height - height) / ycenter; // ybottom
    if (azoomtest < azoom) azoom = azoomtest;
    return azoom;
}

// one coefficient of :2976-3019: predictor, then one corrector step.  a: cdamp or cdamp * 2, q: cquad or cquad * 4; s1 s2: smoothed n - 1,
// n - 2; c0 c1 c2: cumulative n, n - 1, n - 2
static inline float depan_stab_step(float a, float q, float freqnative, float nl, float s1, float s2, float c0, float c1, float c2) {
    float sn = 2 * s1 - s2 -
               a * freqnative * (s1 - s2 - c1 + c2) *
                   (1 + 0.5f * nl / freqnative * fabsf(s1 - s2 - c1 + c2)) -
               q * freqnative * freqnative * (s1 - c1) *
                   (1 + nl * fabsf(s1 - c1));
    sn = 2 * s1 - s2 -
         a * freqnative * 0.5f * (sn - s2 - c0 + c2) *
             (1 + 0.5f * nl / freqnative * 0.5f * fabsf(sn - s2 - c0 + c2)) -
         q * freqnative * freqnative * (s1 - c1) *
             (1 + nl * fabsf(s1 - c1));
    return sn;
}
// the adaptive zoom's predictor and corrector, :3063-3075 and with the slower zf :3080-3092
static inline float depan_stab_zoom_step(float zf, float cdamp, float cquad, float freqnative, float s1, float s2, float a0, float a1, float a2) {
    float sn = 2 * s1 - s2 -
               zf * cdamp * freqnative * (s1 - s2 - a1 + a2)
               - zf * zf * cquad * freqnative * freqnative * (s1 - a1);
    sn = 2 * s1 - s2 -
         zf * cdamp * freqnative * 0.5f * (sn - s2 - a0 + a2)
         - zf * zf * cquad * freqnative * freqnative * (s1 - a1);
    return sn;
}

// MVDepan.cpp:2945-3115.  The arrays are indexed from nbase: element [n - nbase].
static inline void depan_stab_inertial(const DepanStabParams *d, const DepanTransform *trcumul0, int nbase, int ndest, DepanTransform *ptrdif) {
    const int count = ndest - nbase + 1;
    std::vector<DepanTransform> sm(count);
    std::vector<float> az(count), azs(count);
    const DepanStabFrom<const DepanTransform> trcumul = { trcumul0, nbase };
    const DepanStabFrom<DepanTransform> trsmoothed = { sm.data(), nbase };
    const DepanStabFrom<float> azoom = { az.data(), nbase }, azoomsmoothed = { azs.data(), nbase };
    const DepanTransform nonlinfactor = d->nonlinfactor;
    const float freqnative = d->freqnative, pixaspect = d->pixaspect;
    const int nfields = d->nfields;
    DepanTransform trinv, trcur, trtemp;
    depan_set_null(&trsmoothed[nbase]);
    depan_set_null(&trsmoothed[nbase + 1]);
    float cdamp = 12.56f * d->damping / d->fps;
    float cquad = 39.44f / (d->fps * d->fps);
    for (int n = nbase + 2; n <= ndest; n++) {
        trsmoothed[n].dxc = depan_stab_step(cdamp, cquad, freqnative, nonlinfactor.dxc, trsmoothed[n - 1].dxc, trsmoothed[n - 2].dxc, trcumul[n].dxc, trcumul[n - 1].dxc, trcumul[n - 2].dxc);
        trsmoothed[n].dxx = 0.5f * (trcumul[n].dxx + trsmoothed[n - 1].dxx);
        trsmoothed[n].dxy = depan_stab_step(cdamp * 2, cquad * 4, freqnative, nonlinfactor.dxy, trsmoothed[n - 1].dxy, trsmoothed[n - 2].dxy, trcumul[n].dxy, trcumul[n - 1].dxy, trcumul[n - 2].dxy);
        trsmoothed[n].dyx = -trsmoothed[n].dxy * (pixaspect / nfields) * (pixaspect / nfields);
        trsmoothed[n].dyc = depan_stab_step(cdamp, cquad, freqnative, nonlinfactor.dyc, trsmoothed[n - 1].dyc, trsmoothed[n - 2].dyc, trcumul[n].dyc, trcumul[n - 1].dyc, trcumul[n - 2].dyc);
        trsmoothed[n].dyy = trsmoothed[n].dxx;
    }
    if (d->addzoom) {
        azoom[nbase] = d->initzoom;
        azoom[nbase + 1] = d->initzoom;
        azoomsmoothed[nbase] = d->initzoom;
        azoomsmoothed[nbase + 1] = d->initzoom;
        for (int n = nbase + 2; n <= ndest; n++) {
            depan_inversetransform(&trcumul[n], &trinv);
            depan_sumtransform(&trinv, &trsmoothed[n], &trcur);
            azoom[n] = depan_stab_azoom(d, trcur);
            float zf = 1 / (d->cutoff * d->tzoom);
            azoomsmoothed[n] = depan_stab_zoom_step(zf, cdamp, cquad, freqnative, azoomsmoothed[n - 1], azoomsmoothed[n - 2], azoom[n], azoom[n - 1], azoom[n - 2]);
            zf = zf * 0.7f;
            if (azoomsmoothed[n] > azoomsmoothed[n - 1])
                azoomsmoothed[n] = depan_stab_zoom_step(zf, cdamp, cquad, freqnative, azoomsmoothed[n - 1], azoomsmoothed[n - 2], azoom[n], azoom[n - 1], azoom[n - 2]);
            if (azoomsmoothed[n] > 1)
                azoomsmoothed[n] = 1;
            depan_motion2transform(0, 0, 0, azoomsmoothed[n], pixaspect / nfields, d->xcenter, d->ycenter, 1, 1.0, &trtemp);
            depan_sumtransform(&trsmoothed[n], &trtemp, &trsmoothed[n]);
        }
    } else {
        depan_motion2transform(0, 0, 0, d->initzoom, pixaspect / nfields, d->xcenter, d->ycenter, 1, 1.0, &trtemp);
        depan_sumtransform(&trsmoothed[ndest], &trtemp, &trsmoothed[ndest]);
    }
    depan_inversetransform(&trcumul[ndest], &trinv);
    depan_sumtransform(&trinv, &trsmoothed[ndest], ptrdif);
}

// MVDepan.cpp:3118-3246.  trcumul0 is indexed from nbase.
static inline void depan_stab_average(const DepanStabParams *d, const DepanTransform *trcumul0, int nbase, int ndest, int nmax, DepanTransform *ptrdif) {
    const DepanStabFrom<const DepanTransform> trcumul = { trcumul0, nbase };
    std::vector<float> az(nmax - nbase + 1);
    const DepanStabFrom<float> azoom = { az.data(), nbase };
    const float *wint = d->wint.data(), *winfz = d->winfz.data(), *winrz = d->winrz.data();
    const float pixaspect = d->pixaspect;
    const int nfields = d->nfields;
    DepanTransform trsmoothed, trinv, trcur, trtemp;
    float azoomsmoothed;
    int n;
    float norm = 0;
    trsmoothed.dxc = 0;
    trsmoothed.dyc = 0;
    trsmoothed.dxy = 0;
    for (n = nbase; n < ndest; n++) {
        trsmoothed.dxc += trcumul[n].dxc * wint[ndest - n];
        trsmoothed.dyc += trcumul[n].dyc * wint[ndest - n];
        trsmoothed.dxy += trcumul[n].dxy * wint[ndest - n];
        norm += wint[ndest - n];
    }
    for (n = ndest; n <= nmax; n++) {
        trsmoothed.dxc += trcumul[n].dxc * wint[n - ndest];
        trsmoothed.dyc += trcumul[n].dyc * wint[n - ndest];
        trsmoothed.dxy += trcumul[n].dxy * wint[n - ndest];
        norm += wint[n - ndest];
    }
    trsmoothed.dxc /= norm;
    trsmoothed.dyc /= norm;
    trsmoothed.dxy /= norm;
    trsmoothed.dyx = -trsmoothed.dxy * (pixaspect / nfields) * (pixaspect / nfields);
    norm = 0;
    trsmoothed.dxx = 0;
    for (n = (nbase > ndest - 1 ? nbase : ndest - 1); n < ndest; n++) {
        trsmoothed.dxx += trcumul[n].dxx * wint[ndest - n];
        norm += wint[ndest - n];
    }
    for (n = ndest; n <= (nmax < ndest + 1 ? nmax : ndest + 1); n++) {
        trsmoothed.dxx += trcumul[n].dxx * wint[n - ndest];
        norm += wint[n - ndest];
    }
    trsmoothed.dxx /= norm;
    trsmoothed.dyy = trsmoothed.dxx;
    if (d->addzoom) {
        int nbasez = nbase > ndest - d->winfzsize ? nbase : ndest - d->winfzsize;
        int nmaxz = nmax < ndest + d->winrzsize ? nmax : ndest + d->winrzsize;
        azoom[nbasez] = d->initzoom;
        for (n = nbasez + 1; n <= nmaxz; n++) {
            depan_inversetransform(&trcumul[n], &trinv);
            depan_sumtransform(&trinv, &trcumul[n], &trcur);
            azoom[n] = depan_stab_azoom(d, trcur);
        }
        norm = 0;
        azoomsmoothed = 0.0;
        for (n = nbasez; n < ndest; n++) {
            azoomsmoothed += azoom[n] * winfz[ndest - n];
            norm += winfz[ndest - n];
        }
        for (n = ndest; n <= nmaxz; n++) {
            azoomsmoothed += azoom[n] * winrz[n - ndest];
            norm += winrz[n - ndest];
        }
        azoomsmoothed /= norm;
        if (azoomsmoothed > 1)
            azoomsmoothed = 1;
        depan_motion2transform(0, 0, 0, azoomsmoothed, pixaspect / nfields, d->xcenter, d->ycenter, 1, 1.0, &trtemp);
        depan_sumtransform(&trsmoothed, &trtemp, &trsmoothed);
    } else {
        depan_motion2transform(0, 0, 0, d->initzoom, pixaspect / nfields, d->xcenter, d->ycenter, 1, 1.0, &trtemp);
        depan_sumtransform(&trsmoothed, &trtemp, &trsmoothed);
    }
    depan_inversetransform(&trcumul[ndest], &trinv);
    depan_sumtransform(&trinv, &trsmoothed, ptrdif);
}

// MVDepan.cpp:3249-3329
static inline void depan_stab_limit(const DepanStabParams *d, float *dxdif, float *dydif, float *zoomdif, float *rotdif, int ndest, int *nbase) {
    const float initzoom = d->initzoom, dxmax = d->dxmax, dymax = d->dymax, zoommax = d->zoommax, rotmax = d->rotmax;
#define DEPAN_STAB_RESET() do { *dxdif = 0; *dydif = 0; *zoomdif = initzoom; *rotdif = 0; *nbase = ndest; } while (0)
    if (!(isfinite(*dxdif))) DEPAN_STAB_RESET();
    else if (fabsf(*dxdif) > fabsf(dxmax)) {
        if (dxmax >= 0) *dxdif = *dxdif >= 0 ? sqrt(*dxdif * dxmax) : -sqrt(-*dxdif * dxmax);
        else DEPAN_STAB_RESET();
    }
    if (!(isfinite(*dydif))) DEPAN_STAB_RESET();
    else if (fabsf(*dydif) > fabsf(dymax)) {
        if (dymax >= 0) *dydif = *dydif >= 0 ? sqrt(*dydif * dymax) : -sqrt(-*dydif * dymax);
        else DEPAN_STAB_RESET();
    }
    if (!(isfinite(*zoomdif))) DEPAN_STAB_RESET();
    else if (fabsf(*zoomdif - 1) > fabsf(zoommax) - 1) {
        if (zoommax >= 0) *zoomdif = *zoomdif >= 1 ? 1 + sqrt(fabsf(*zoomdif - 1) * fabsf(zoommax - 1)) : 1 - sqrt(fabsf(*zoomdif - 1) * fabsf(zoommax - 1));
        else DEPAN_STAB_RESET();
    }
    if (!(isfinite(*rotdif))) DEPAN_STAB_RESET();
    else if (fabsf(*rotdif) > fabsf(rotmax)) {
        if (rotmax >= 0) *rotdif = *rotdif >= 0 ? sqrt(*rotdif * rotmax) : -sqrt(-*rotdif * rotmax);
        else DEPAN_STAB_RESET();
    }
#undef DEPAN_STAB_RESET
}

// the frames of the request sets, :3567-3591 (method 0) and :3717-3763 (method 1): the data frames whose motion a plan may read and the clip
// frames it may name.  Method 1 with next > radius: fillBorderNext reads data frames up to ndest + next although the reference's last
// request loop (:3757) is empty; they are part of the window here.
static inline int depan_stab_first_base(const DepanStabParams *d, int ndest) {
    if (d->method == 1) return ndest - d->radius > 0 ? ndest - d->radius : 0;
    const float v = ndest - 10 * d->fps / d->cutoff;
    return v > 0 ? (int)v : 0; // v <= ndest; NaN and negative values give 0
}
static inline void depan_stab_window(const DepanStabParams *d, int ndest, int *data_first, int *data_last, int *clip_first, int *clip_last) {
    const int last = d->num_frames - 1;
    const int nbase = depan_stab_first_base(d, ndest);
    const long long want = (long long)ndest + d->next;
    const int nnext = d->next ? (int)(want < last ? want : last) : ndest;
    int dl = nnext;
    if (d->method == 1) { const long long m = (long long)ndest + d->radius; const int nmax = (int)(m < last ? m : last); if (nmax > dl) dl = nmax; }
    *data_first = nbase; *data_last = dl;
    const long long p = (long long)ndest - d->prev;
    *clip_first = d->prev ? (int)(p > nbase ? p : nbase) : ndest;
    *clip_last = nnext;
}

struct DepanStabSource { int used, frame; DepanTransform tr; };
struct DepanStabPlan {
    DepanTransform tr;       // the luma transform of clip frame ndest
    int nbase, base;         // the final base; base: nbase == ndest, "BASE!" in the info string
    float motion[4];         // dx, dy, zoom, rot of the info string, :3700 / :3876
    DepanStabSource prev, next;
};

// fillBorderPrev's source, :3398-3419: always frame nprev, with the transform summed over nprev + 1 .. ndest (the assignment of :3412 is
// unconditional, so the "most centred and nearest" test of :3415-3418 selects nothing and is not computed here)
static inline void depan_stab_prev(const DepanStabParams *d, const DepanStabMotions &M, int nbase, int ndest, const DepanTransform *trdif, DepanStabSource *s) {
    const long long p = (long long)ndest - d->prev;
    const int nprev = (int)(p < nbase ? nbase : p);
    DepanTransform tr0 = *trdif, trcur;
    for (int n = ndest - 1; n >= nprev; n--) {
        depan_stab_frame_transform(d, M, n + 1, &trcur);
        depan_sumtransform(&tr0, &trcur, &tr0);
    }
    s->used = 1; s->frame = nprev; s->tr = tr0;
}

// fillBorderNext's source, :3461-3502.  The transform is the one accumulated over every frame the walk passed, also where an earlier frame
// was chosen; a bad frame ends the walk at the frame before it.
static inline void depan_stab_next(const DepanStabParams *d, const DepanStabMotions &M, int ndest, const DepanTransform *trdif, DepanStabSource *s) {
    float dxt1, dyt1, rott1, zoomt1;
    const long long want = (long long)ndest + d->next;
    const int nnext = (int)(want >= d->num_frames ? d->num_frames - 1 : want);
    int nnextbest = nnext;
    float dabsmin = 1000;
    DepanTransform tr0 = *trdif, trcur, trinv;
    for (int n = ndest + 1; n <= nnext; n++) {
        if (M.x(n) != DEPAN_MOTIONBAD) {
            depan_stab_frame_transform(d, M, n, &trcur);
            depan_inversetransform(&trcur, &trinv);
            depan_sumtransform(&trinv, &tr0, &tr0);
            depan_transform2motion(&tr0, 1, d->xcenter, d->ycenter, d->pixaspect / d->nfields, &dxt1, &dyt1, &rott1, &zoomt1);
            if ((fabs(dxt1) + fabs(dyt1) + n - ndest) < dabsmin) {
                dabsmin = fabs(dxt1) + fabs(dyt1) + n - ndest;
                nnextbest = n;
            }
        } else {
            nnextbest = n - 1;
            break;
        }
    }
    s->used = 1; s->frame = nnextbest; s->tr = tr0;
}

static inline void depan_stab_one_nan(float *v, int n) {
    const uint32_t q = 0x7FC00000u;
    for (int i = 0; i < n; i++) if (v[i] != v[i]) memcpy(&v[i], &q, 4);
}

// one output frame: depanStabiliseGetFrame0 :3567-3666 / depanStabiliseGetFrame1 :3717-3841, then the two selections.  motions: dx, dy, zoom,
// rot of the data frames of depan_stab_window, data_first first.
static inline void depan_stab_plan(const DepanStabParams *d, int ndest, const float *motions, DepanStabPlan *out) {
    int nbase = depan_stab_first_base(d, ndest);
    const DepanStabMotions M = { motions, nbase };
    const float pa = d->pixaspect / d->nfields;
    float dxdif, dydif, zoomdif, rotdif;
    DepanTransform trdif, trcur;
    if (d->method == 0) {
        for (int n = ndest; n >= nbase; n--)
            if (M.x(n) == DEPAN_MOTIONBAD) { if (n > nbase) nbase = n; break; }
        if (nbase == ndest) {
            depan_motion2transform(0, 0, 0, d->initzoom, pa, d->xcenter, d->ycenter, 1, 1.0f, &trdif);
        } else {
            std::vector<DepanTransform> trcumul(ndest - nbase + 1);
            depan_set_null(&trcumul[0]);
            for (int n = nbase + 1; n <= ndest; n++) {
                depan_stab_frame_transform(d, M, n, &trcur);
                depan_sumtransform(&trcumul[n - nbase - 1], &trcur, &trcumul[n - nbase]);
            }
            depan_stab_inertial(d, trcumul.data(), nbase, ndest, &trdif);
            depan_transform2motion(&trdif, 1, d->xcenter, d->ycenter, pa, &dxdif, &dydif, &rotdif, &zoomdif);
            if (d->num_frames < (long long)d->fitlast + ndest + 1) {
                float endFactor = ((float)(d->num_frames - ndest - 1)) / d->fitlast;
                dxdif *= endFactor;
                dydif *= endFactor;
                rotdif *= endFactor;
                zoomdif = d->initzoom + (zoomdif - d->initzoom) * endFactor;
            }
            depan_stab_limit(d, &dxdif, &dydif, &zoomdif, &rotdif, ndest, &nbase);
            depan_motion2transform(dxdif, dydif, rotdif, zoomdif, pa, d->xcenter, d->ycenter, 1, 1.0f, &trdif);
        }
    } else {
        const long long m = (long long)ndest + d->radius;
        int nmax = (int)(m < d->num_frames - 1 ? m : d->num_frames - 1);
        for (int n = ndest; n >= nbase; n--)
            if (M.x(n) == DEPAN_MOTIONBAD) { if (n > nbase) nbase = n; break; }
        for (int n = ndest + 1; n <= nmax; n++)
            if (M.x(n) == DEPAN_MOTIONBAD) { if (n < nmax) nmax = n - 1 > ndest ? n - 1 : ndest; break; }
        const int smaller_distance = nmax - ndest < ndest - nbase ? nmax - ndest : ndest - nbase;
        nmax = ndest + smaller_distance;
        nbase = ndest - smaller_distance;
        std::vector<DepanTransform> trcumul(nmax - nbase + 1);
        depan_set_null(&trcumul[0]);
        for (int n = nbase + 1; n <= nmax; n++) {
            depan_stab_frame_transform(d, M, n, &trcur);
            depan_sumtransform(&trcumul[n - nbase - 1], &trcur, &trcumul[n - nbase]);
        }
        depan_stab_average(d, trcumul.data(), nbase, ndest, nmax, &trdif);
        depan_transform2motion(&trdif, 1, d->xcenter, d->ycenter, pa, &dxdif, &dydif, &rotdif, &zoomdif);
        depan_motion2transform(dxdif, dydif, rotdif, zoomdif, pa, d->xcenter, d->ycenter, 1, 1.0f, &trdif);
    }
    memset(out, 0, sizeof(*out));
    out->tr = trdif; out->nbase = nbase; out->base = nbase == ndest;
    if (d->prev > 0) depan_stab_prev(d, M, nbase, ndest, &trdif, &out->prev);
    if (d->next > 0) depan_stab_next(d, M, ndest, &trdif, &out->next);
    depan_transform2motion(&trdif, 1, d->xcenter, d->ycenter, pa, &out->motion[0], &out->motion[1], &out->motion[3], &out->motion[2]);
    // IEEE 754 leaves the sign and payload of a NaN result open and a compiler may commute the operands of + and *, so which NaN the reference's
    // own arithmetic ends on depends on its build.  A plan carries one: the positive quiet NaN.  (No NaN's bits ever reach a number.)
    depan_stab_one_nan(&out->tr.dxc, 6); depan_stab_one_nan(out->motion, 4); depan_stab_one_nan(&out->prev.tr.dxc, 6); depan_stab_one_nan(&out->next.tr.dxc, 6);
}
