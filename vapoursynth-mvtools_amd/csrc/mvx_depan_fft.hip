// mvx_depan_fft.hip -- DepanEstimate on gfx950 (MVDepan.cpp:618-1503): pan and zoom between consecutive frames from the peak of the
// cross-correlation of one or two luma windows, computed with a power-of-two real 2-D FFT in LDS.  The reference calls FFTW; here the
// transforms are radix-2 kernels over tables of twiddles that the host computes in double and rounds once (no sine or cosine on the device,
// no fast-math, no FMA contraction).  The text of the passes is mvx_depan_fft_core.h, which a host compiler runs too.
//   stage 1, mvx_depan_estimate_spectra  : de_rows_kernel (two window rows per complex transform), de_cols_kernel (in place)
//   stage 2, mvx_depan_estimate_correlate: de_correlate_kernel (conjugate product on load, inverse columns, kept rows only), de_rows_inverse_kernel,
//                                          de_peak_kernel, then the host tail (mvx_depan_estimate_host.h)
//            mvx_depan_estimate_correlate_show: the same, then the two inverse passes again with every row kept, de_minmax_kernel, de_paint_kernel
//   stage 3, mvx_depan_estimate_finish   : host only
// A batch is one launch per pass: blockIdx.x covers job x window x group of rows or columns.  No atomics: every sum has a fixed order (the mean's
// is the reference's serial one), so the results are the same from run to run and for any batch size.  A workgroup holds at most 8192 complex values, 64 KiB of LDS.
#include <math.h>
#include <algorithm>
#include "mvx_common.h"
#include "mvx_depan_estimate_host.h"
#include "mvx_depan_fft_core.h"

struct DEJob { const unsigned char *a; const unsigned char *b; unsigned char *out; };

extern __shared__ float de_lds[];

// grid: job x window x groups
__global__ __launch_bounds__(DE_THREADS) void de_rows_kernel(DEParams P, const DEJob *jobs, const DEComplex *twx, int groups) {
    const int g = blockIdx.x % groups, jw = blockIdx.x / groups, win = jw % P.nwin, job = jw / P.nwin;
    float *re = de_lds, *im = de_lds + (P.winx << P.lgcx);
    DEComplex *spec = (DEComplex *)jobs[job].out + (long long)win * P.winy * P.nx;
    de_rows_forward(P, jobs[job].a, win, g, spec, twx, re, im);
}

__global__ __launch_bounds__(DE_THREADS) void de_cols_kernel(DEParams P, const DEJob *jobs, const DEComplex *twy, int groups) {
    const int g = blockIdx.x % groups, jw = blockIdx.x / groups, win = jw % P.nwin, job = jw / P.nwin;
    float *re = de_lds, *im = de_lds + (P.winy << P.lgcy);
    de_cols_forward(P, g, (DEComplex *)jobs[job].out + (long long)win * P.winy * P.nx, twy, re, im);
}

// half: [job][window][kept row][nx]
__global__ __launch_bounds__(DE_THREADS) void de_correlate_kernel(DEParams P, const DEJob *jobs, const DEComplex *twy, int groups, DEComplex *half) {
    const int g = blockIdx.x % groups, jw = blockIdx.x / groups, win = jw % P.nwin, job = jw / P.nwin;
    float *re = de_lds, *im = de_lds + (P.winy << P.lgcy);
    const long long off = (long long)win * P.winy * P.nx;
    de_cols_correlate(P, g, (const DEComplex *)jobs[job].b + off, (const DEComplex *)jobs[job].a + off, half + (long long)jw * P.nrows * P.nx, twy, re, im);
}

// corr: [job][window][kept row][winx]
__global__ __launch_bounds__(DE_THREADS) void de_rows_inverse_kernel(DEParams P, const DEComplex *twx, int groups, const DEComplex *half, float *corr) {
    const int g = blockIdx.x % groups, jw = blockIdx.x / groups;
    float *re = de_lds, *im = de_lds + (P.winx << P.lgcx);
    de_rows_inverse(P, g, half + (long long)jw * P.nrows * P.nx, corr + (long long)jw * P.nrows * P.winx, twx, re, im);
}

__global__ __launch_bounds__(DE_THREADS) void de_peak_kernel(DEParams P, const float *corr, DEScan *scans) {
    __shared__ float stage[2 * DE_CHUNK];
    __shared__ float lmax[DE_THREADS];
    __shared__ int lidx[DE_THREADS];
    de_peak(P, corr + (long long)blockIdx.x * P.nrows * P.winx, scans + blockIdx.x, stage, lmax, lidx);
}

// show.  grid: job x window x groups; full: [job][window][winy][winx]; partial: [job][window][groups][2]
__global__ __launch_bounds__(DE_THREADS) void de_minmax_kernel(DEParams P, const float *full, int groups, float *partial) {
    __shared__ float lmin[DE_THREADS];
    __shared__ float lmax[DE_THREADS];
    const int g = blockIdx.x % groups, jw = blockIdx.x / groups;
    de_minmax(P, full + (long long)jw * P.winy * P.winx, g, groups, partial + (long long)jw * groups * 2, lmin, lmax);
}

__global__ __launch_bounds__(DE_THREADS) void de_paint_kernel(DEParams P, const DEJob *jobs, const float *full, int groups, const float *partial, int pixel_max) {
    __shared__ float lmin[DE_THREADS];
    __shared__ float lmax[DE_THREADS];
    const int g = blockIdx.x % groups, jw = blockIdx.x / groups, win = jw % P.nwin, job = jw / P.nwin;
    de_paint(P, full + (long long)jw * P.winy * P.winx, partial + (long long)jw * groups * 2, g, groups, jobs[job].out, win, pixel_max, lmin, lmax);
}

// ------------------------------------------------------------------------------------------------ host object

struct mvx_depan_estimate {
    CallGuard guard;
    DepanEstimateParams E;
    DEParams P;
    std::vector<DEComplex> twx, twy;   // exp(-2 pi i k / n), k < n / 2: computed in double, rounded once
    DevBuf<DEComplex> dTwx, dTwy;
    bool twiddles_up = false;
    DevBuf<DEJob> dJobs;
    DevBuf<DEComplex> dHalf;
    DevBuf<float> dCorr;
    DevBuf<DEScan> dScans;
    DevBuf<DEComplex> dHalfFull;       // show: the surface with every row kept
    DevBuf<float> dCorrFull, dMinMax;
};

static_assert(sizeof(DEScan) == sizeof(mvx_depan_estimate_scan) && sizeof(DepanEstimateScan) == sizeof(DEScan), "layouts");
static_assert(sizeof(DepanEstimateResult) == sizeof(mvx_depan_estimate_result), "layouts");

// MVDepan.cpp:1271-1433 depanEstimateCreate
extern "C" __attribute__((visibility("default"))) int mvx_depan_estimate_create(const mvx_depan_estimate_args *a, const mvx_depan_clip *clip, int num_frames,
        mvx_depan_estimate **out, char *err) {
    MVX_CREATE_BEGIN(out);
    DepanEstimateParams E;
    memset(&E, 0, sizeof(E));
    E.trust_limit = (float)a->trust; E.zoommax = (float)a->zoommax; E.stab = (float)a->stab; E.pixaspect = (float)a->pixaspect;
    E.winx = a->winx == MVX_UNSET ? 0 : a->winx; E.winy = a->winy == MVX_UNSET ? 0 : a->winy;
    E.wleft = a->wleft == MVX_UNSET ? -1 : a->wleft; E.wtop = a->wtop == MVX_UNSET ? -1 : a->wtop;
    E.dxmax = a->dxmax == MVX_UNSET ? -1 : a->dxmax; E.dymax = a->dymax == MVX_UNSET ? -1 : a->dymax;
    E.fields = a->fields == MVX_UNSET ? 0 : !!a->fields;
    E.tff_exists = a->tff != MVX_UNSET; E.tff = E.tff_exists ? !!a->tff : 0;
    E.width = clip->width; E.height = clip->height; E.bits = clip->bits; E.num_frames = num_frames;
    if (const char *msg = depan_estimate_resolve(&E, a->float_samples != 0)) MVX_FAIL("%s", msg);
    mvx_depan_estimate *h = new mvx_depan_estimate();
    h->E = E;
    DEParams &P = h->P;
    memset(&P, 0, sizeof(P));
    P.winx = E.winx; P.winy = E.winy; P.nx = E.winx / 2 + 1;
    P.lgx = mvx_ilog2(E.winx); P.lgy = mvx_ilog2(E.winy);
    P.cx = de_batch(E.winx); P.lgcx = mvx_ilog2(P.cx); P.cy = de_batch(E.winy); P.lgcy = mvx_ilog2(P.cy);
    P.nwin = E.nwin; P.wleft[0] = E.wleft; P.wleft[1] = E.wleft + E.width / 2; P.wtop = E.wtop;
    P.dxmax = E.dxmax; P.dymax = E.dymax;
    P.nrows = std::min(E.winy, 2 * E.dymax + 3); P.jshift = E.winy - P.nrows;
    P.bits16 = E.bits > 8;
    h->twx.resize(E.winx / 2); h->twy.resize(E.winy / 2);
    de_twiddles(h->twx.data(), E.winx);
    de_twiddles(h->twy.data(), E.winy);
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) void mvx_depan_estimate_destroy(mvx_depan_estimate *h) { delete h; }

extern "C" __attribute__((visibility("default"))) void mvx_depan_estimate_get_info(const mvx_depan_estimate *h, mvx_depan_estimate_info *info) {
    const DepanEstimateParams &E = h->E;
    info->winx = E.winx; info->winy = E.winy; info->wleft = E.wleft; info->wtop = E.wtop; info->dxmax = E.dxmax; info->dymax = E.dymax;
    info->windows = E.nwin;
    info->spectrum_bytes = (int64_t)E.winy * (E.winx / 2 + 1) * 8; // fftsize, :1431-1433
}

static int de_upload_twiddles(mvx_depan_estimate *h, hipStream_t st) {
    if (h->twiddles_up) return MVX_OK;
    // 64 KiB of dynamic LDS at the longest transforms
    HIP_CHECK(hipFuncSetAttribute((const void *)de_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DE_LDS_COMPLEX * 8));
    HIP_CHECK(hipFuncSetAttribute((const void *)de_cols_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DE_LDS_COMPLEX * 8));
    HIP_CHECK(hipFuncSetAttribute((const void *)de_correlate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DE_LDS_COMPLEX * 8));
    HIP_CHECK(hipFuncSetAttribute((const void *)de_rows_inverse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DE_LDS_COMPLEX * 8));
    HIP_CHECK(h->dTwx.reserve(h->twx.size()));
    HIP_CHECK(h->dTwy.reserve(h->twy.size()));
    HIP_CHECK(hipMemcpyAsync(h->dTwx.p, h->twx.data(), sizeof(DEComplex) * h->twx.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(h->dTwy.p, h->twy.data(), sizeof(DEComplex) * h->twy.size(), hipMemcpyHostToDevice, st));
    h->twiddles_up = true;
    return MVX_OK;
}

#define DE_MAX_JOBS 4096

// stage 1, :956-997
extern "C" __attribute__((visibility("default"))) int mvx_depan_estimate_spectra(mvx_depan_estimate *h, int nframes, const void *const *luma_planes, ptrdiff_t pitch,
        void *const *spectra_out, void *stream) {
    if (nframes <= 0) return MVX_OK;
    const DepanEstimateParams &E = h->E;
    if (nframes > DE_MAX_JOBS) { mvx_set_error("mvx_depan_estimate_spectra: at most %d frames per call", DE_MAX_JOBS); return MVX_E_ARG; }
    const int bps = E.bits > 8 ? 2 : 1;
    if (pitch % bps || pitch < (ptrdiff_t)E.width * bps) { mvx_set_error("mvx_depan_estimate_spectra: the pitch must hold a row and be a multiple of the sample size"); return MVX_E_ARG; }
    std::vector<DEJob> hj(nframes);
    for (int f = 0; f < nframes; f++) {
        hj[f].a = (const unsigned char *)luma_planes[f]; hj[f].b = nullptr; hj[f].out = (unsigned char *)spectra_out[f];
        if (!hj[f].a || !hj[f].out) { mvx_set_error("mvx_depan_estimate_spectra: every frame needs its luma plane and room for its spectra"); return MVX_E_ARG; }
    }
    hipStream_t st = (hipStream_t)stream;
    CallGuard::Scope scope(h->guard, st);
    if (int rc = de_upload_twiddles(h, st)) return rc;
    DEParams P = h->P;
    P.pitch = pitch;
    HIP_CHECK(h->dJobs.reserve(nframes));
    HIP_CHECK(hipMemcpyAsync(h->dJobs.p, hj.data(), sizeof(DEJob) * nframes, hipMemcpyHostToDevice, st));
    const int rgroups = (P.winy / 2 + P.cx - 1) / P.cx, cgroups = (P.nx + P.cy - 1) / P.cy;
    hipLaunchKernelGGL(de_rows_kernel, dim3((unsigned)(nframes * P.nwin * rgroups)), dim3(DE_THREADS), (size_t)(P.winx << P.lgcx) * 8, st, P, h->dJobs.p, h->dTwx.p, rgroups);
    hipLaunchKernelGGL(de_cols_kernel, dim3((unsigned)(nframes * P.nwin * cgroups)), dim3(DE_THREADS), (size_t)(P.winy << P.lgcy) * 8, st, P, h->dJobs.p, h->dTwy.p, cgroups);
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}

static int de_tail(const mvx_depan_estimate *h, int npairs, const DepanEstimateScan *scans, const int32_t *top_field, const int32_t *frame_numbers,
                   mvx_depan_estimate_result *out) {
    for (int i = 0; i < npairs; i++) {
        const int tf = top_field && top_field[i] != MVX_UNSET ? !!top_field[i] : -1;
        if (!depan_estimate_pair(h->E, scans + (size_t)i * h->E.nwin, tf, frame_numbers ? frame_numbers[i] : 1, (DepanEstimateResult *)&out[i])) {
            mvx_set_error("DepanEstimate: _Field property not found in input frame. Therefore, you must pass tff argument.");
            return MVX_E_ARG;
        }
    }
    return MVX_OK;
}

extern "C" __attribute__((visibility("default"))) int mvx_depan_estimate_host_tail(const mvx_depan_estimate *h, int npairs, const mvx_depan_estimate_scan *scans,
        const int32_t *top_field, const int32_t *frame_numbers, mvx_depan_estimate_result *out) {
    if (npairs <= 0) return MVX_OK;
    return de_tail(h, npairs, (const DepanEstimateScan *)scans, top_field, frame_numbers, out);
}

// stage 2, :1000-1148.  Synchronous: the scan results come back to the host for the tail.  With show_planes the correlation surface is painted too
// (:1072-1077, :1123-1124): the scan above stays on its kept rows, whose pairing in de_rows_inverse decides their floats, and the two inverse passes run
// once more with every row kept for the minimum, the maximum and the paint alone.
static int de_correlate(const char *name, mvx_depan_estimate *h, int npairs, const void *const *prev_spectra, const void *const *cur_spectra, const int32_t *top_field,
        const int32_t *frame_numbers, mvx_depan_estimate_result *out, mvx_depan_estimate_scan *scans_out, void *const *show_planes, ptrdiff_t show_pitch, void *stream) {
    if (npairs <= 0) return MVX_OK;
    if (npairs > DE_MAX_JOBS) { mvx_set_error("%s: at most %d pairs per call", name, DE_MAX_JOBS); return MVX_E_ARG; }
    if (show_planes) {
        const int bps = h->E.bits > 8 ? 2 : 1;
        if (show_pitch % bps || show_pitch < (ptrdiff_t)h->E.width * bps) { mvx_set_error("%s: the pitch must hold a row and be a multiple of the sample size", name); return MVX_E_ARG; }
    }
    std::vector<DEJob> hj(npairs);
    for (int f = 0; f < npairs; f++) {
        hj[f].a = (const unsigned char *)prev_spectra[f]; hj[f].b = (const unsigned char *)cur_spectra[f]; hj[f].out = show_planes ? (unsigned char *)show_planes[f] : nullptr;
        if (!hj[f].a || !hj[f].b) { mvx_set_error("%s: every pair needs both spectra", name); return MVX_E_ARG; }
        if (show_planes && !hj[f].out) { mvx_set_error("%s: every pair needs its luma plane", name); return MVX_E_ARG; }
    }
    const DEParams &P = h->P;
    const size_t nscan = (size_t)npairs * P.nwin;
    std::vector<DepanEstimateScan> scans(nscan);
    {
        hipStream_t st = (hipStream_t)stream;
        CallGuard::Scope scope(h->guard, st);
        if (int rc = de_upload_twiddles(h, st)) return rc;
        HIP_CHECK(h->dJobs.reserve(npairs));
        HIP_CHECK(h->dHalf.reserve(nscan * P.nrows * P.nx));
        HIP_CHECK(h->dCorr.reserve(nscan * P.nrows * P.winx));
        HIP_CHECK(h->dScans.reserve(nscan));
        HIP_CHECK(hipMemcpyAsync(h->dJobs.p, hj.data(), sizeof(DEJob) * npairs, hipMemcpyHostToDevice, st));
        const int cgroups = (P.nx + P.cy - 1) / P.cy, rgroups = ((P.nrows + 1) / 2 + P.cx - 1) / P.cx;
        hipLaunchKernelGGL(de_correlate_kernel, dim3((unsigned)(nscan * cgroups)), dim3(DE_THREADS), (size_t)(P.winy << P.lgcy) * 8, st, P, h->dJobs.p, h->dTwy.p, cgroups, h->dHalf.p);
        hipLaunchKernelGGL(de_rows_inverse_kernel, dim3((unsigned)(nscan * rgroups)), dim3(DE_THREADS), (size_t)(P.winx << P.lgcx) * 8, st, P, h->dTwx.p, rgroups, h->dHalf.p, h->dCorr.p);
        hipLaunchKernelGGL(de_peak_kernel, dim3((unsigned)nscan), dim3(DE_THREADS), 0, st, P, h->dCorr.p, h->dScans.p);
        if (show_planes) {
            DEParams F = P;                       // every row of the surface
            F.nrows = F.winy; F.jshift = 0; F.pitch = show_pitch;
            const int fgroups = (F.winy / 2 + F.cx - 1) / F.cx, sgroups = de_show_groups(F.winx * F.winy);
            HIP_CHECK(h->dHalfFull.reserve(nscan * F.winy * F.nx));
            HIP_CHECK(h->dCorrFull.reserve(nscan * F.winy * F.winx));
            HIP_CHECK(h->dMinMax.reserve(nscan * sgroups * 2));
            hipLaunchKernelGGL(de_correlate_kernel, dim3((unsigned)(nscan * cgroups)), dim3(DE_THREADS), (size_t)(F.winy << F.lgcy) * 8, st, F, h->dJobs.p, h->dTwy.p, cgroups, h->dHalfFull.p);
            hipLaunchKernelGGL(de_rows_inverse_kernel, dim3((unsigned)(nscan * fgroups)), dim3(DE_THREADS), (size_t)(F.winx << F.lgcx) * 8, st, F, h->dTwx.p, fgroups, h->dHalfFull.p, h->dCorrFull.p);
            hipLaunchKernelGGL(de_minmax_kernel, dim3((unsigned)(nscan * sgroups)), dim3(DE_THREADS), 0, st, F, h->dCorrFull.p, sgroups, h->dMinMax.p);
            hipLaunchKernelGGL(de_paint_kernel, dim3((unsigned)(nscan * sgroups)), dim3(DE_THREADS), 0, st, F, h->dJobs.p, h->dCorrFull.p, sgroups, h->dMinMax.p, (1 << h->E.bits) - 1);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(scans.data(), h->dScans.p, sizeof(DEScan) * nscan, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (scans_out) memcpy(scans_out, scans.data(), sizeof(DEScan) * nscan);
    return de_tail(h, npairs, scans.data(), top_field, frame_numbers, out);
}

extern "C" __attribute__((visibility("default"))) int mvx_depan_estimate_correlate(mvx_depan_estimate *h, int npairs, const void *const *prev_spectra, const void *const *cur_spectra,
        const int32_t *top_field, const int32_t *frame_numbers, mvx_depan_estimate_result *out, mvx_depan_estimate_scan *scans_out, void *stream) {
    return de_correlate("mvx_depan_estimate_correlate", h, npairs, prev_spectra, cur_spectra, top_field, frame_numbers, out, scans_out, nullptr, 0, stream);
}

extern "C" __attribute__((visibility("default"))) int mvx_depan_estimate_correlate_show(mvx_depan_estimate *h, int npairs, const void *const *prev_spectra,
        const void *const *cur_spectra, const int32_t *top_field, const int32_t *frame_numbers, mvx_depan_estimate_result *out, mvx_depan_estimate_scan *scans_out,
        void *const *show_planes, ptrdiff_t show_pitch, void *stream) {
    if (npairs > 0 && !show_planes) { mvx_set_error("mvx_depan_estimate_correlate_show: every pair needs its luma plane"); return MVX_E_ARG; }
    return de_correlate("mvx_depan_estimate_correlate_show", h, npairs, prev_spectra, cur_spectra, top_field, frame_numbers, out, scans_out, show_planes, show_pitch, stream);
}

// stage 3, :1154-1243
extern "C" __attribute__((visibility("default"))) int mvx_depan_estimate_finish(const mvx_depan_estimate *h, int n, const mvx_depan_estimate_result results_prev_cur_next[3],
        mvx_depan_motion *motion) {
    float m[4];
    depan_estimate_finish(h->E, n, (const DepanEstimateResult *)results_prev_cur_next, m);
    motion->dx = m[0]; motion->dy = m[1]; motion->zoom = m[2]; motion->rot = m[3];
    motion->iter = 0; motion->error = 0.0f;
    return MVX_OK;
}
