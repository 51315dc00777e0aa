// mvx_depan.hip -- DepanAnalyse on gfx950 (MVDepan.cpp:41-615).  DepanCompensate and DepanStabilise are in mvx_depan_warp.hip.
//
// depan_gather_kernel writes the verdict of fgopIsUsable, the level-0 records and the mask byte under every block centre of all jobs into a
// staging buffer; the estimator (mvx_depan_host.h) runs on the host, in block order, because every one of its sums is a serial float chain.
#include <math.h>
#include "mvx_fps_shared.h"
#include "mvx_depan_host.h"

struct DGParams { int nBlk, nBlkX, nLvCount, stepX, stepY, halfX, halfY, width, height; long long thscd1; int thscd2; long long maskPitch, stride; };
struct DGJob { const unsigned char *blob, *mask; };

// per job: [0] the verdict, then from byte 16 nBlk records, then nBlk ints of mask bytes (-1: none); one workgroup per job
__global__ __launch_bounds__(256) void depan_gather_kernel(DGParams P, const DGJob *jobs, unsigned char *staging) {
    const DGJob J = jobs[blockIdx.x];
    unsigned char *out = staging + blockIdx.x * P.stride;
    const bool usable = fps_block_usable(J.blob, J.blob != nullptr, P.nLvCount, P.nBlk, P.thscd1, P.thscd2);
    if (threadIdx.x == 0) *(int *)out = usable ? 1 : 0;
    GVecD *rec = (GVecD *)(out + 16);
    int *maskv = (int *)(out + 16 + (size_t)P.nBlk * 16);
    const GVecD *vec = J.blob ? mvx_level0(J.blob, P.nLvCount) : nullptr;
    for (int n = threadIdx.x; n < P.nBlk; n += 256) {
        GVecD r = { 0, 0, 0 };
        if (vec) r = vec[n];
        rec[n] = r;
        const int j = n / P.nBlkX, i = n - j * P.nBlkX;
        const int bx = i * P.stepX + P.halfX, by = j * P.stepY + P.halfY;
        maskv[n] = (J.mask && bx < P.width && by < P.height) ? J.mask[bx + by * P.maskPitch] : -1; // MVDepan.cpp:309-312
    }
}

struct mvx_depan_analyse {
    CallGuard guard;
    DepanAnalyseParams P;
    DevBuf<DGJob> dJobs;
    DevBuf<unsigned char> dStaging;
};

// MVDepan.cpp:473-615 depanAnalyseCreate
extern "C" __attribute__((visibility("default"))) int mvx_depan_analyse_create(const mvx_depan_analyse_args *a, const mvx_analysis_data *ad, const mvx_depan_clip *clip,
        const mvx_depan_clip *mask, int num_frames, int vector_frames, int mask_frames, mvx_depan_analyse **out, char *err) {
    MVX_CREATE_BEGIN(out);
    const float pixaspect = (float)a->pixaspect;
    int64_t thscd1; int32_t thscd2;
    if (pixaspect <= 0.0f) MVX_FAIL("DepanAnalyse: pixaspect must be positive.");
    if (num_frames > vector_frames) MVX_FAIL("DepanAnalyse: vectors must have at least as many frames as clip.");
    if (mask) { // the reference names DepanStabilise in these two messages
        if (num_frames > mask_frames) MVX_FAIL("DepanStabilise: mask must have at least as many frames as clip.");
        if (mask->width != clip->width || mask->height != clip->height || mask->bits > 8)
            MVX_FAIL("DepanStabilise: mask must have constant format, the same dimensions as clip, and no more than 8 bits per sample.");
    }
    if (ad->nDeltaFrame != 1) MVX_FAIL("DepanAnalyse: vectors clip must be created with delta=1."); // :579-580 overwrites the message of scaleThSCD
    if (int rc = mvx_resolve_thscd("DepanAnalyse", a->thscd1, a->thscd2, ad, &thscd1, &thscd2, err)) return rc;
    mvx_depan_analyse *h = new mvx_depan_analyse();
    DepanAnalyseParams &P = h->P;
    memset(&P, 0, sizeof(P));
    P.nBlkX = ad->nBlkX; P.nBlkY = ad->nBlkY; P.nBlkSizeX = ad->nBlkSizeX; P.nBlkSizeY = ad->nBlkSizeY;
    P.stepX = ad->nBlkSizeX - ad->nOverlapX; P.stepY = ad->nBlkSizeY - ad->nOverlapY;
    P.nPel = ad->nPel; P.nLvCount = ad->nLvCount; P.isBackward = ad->isBackward;
    P.width = clip->width; P.height = clip->height;
    P.zoom = a->zoom == MVX_UNSET ? 1 : !!a->zoom; P.rot = a->rot == MVX_UNSET ? 1 : !!a->rot;
    P.fields = a->fields == MVX_UNSET ? 0 : !!a->fields;
    P.hasMask = mask ? 1 : 0;
    P.pixaspect = pixaspect; P.error = (float)a->error; P.wrong = (float)a->wrong; P.zerow = (float)a->zerow;
    P.thscd1 = thscd1; P.thscd2 = thscd2;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) void mvx_depan_analyse_destroy(mvx_depan_analyse *h) { delete h; }

static_assert(sizeof(DepanMotion) == sizeof(mvx_depan_motion) && sizeof(DepanGather) == 16 && sizeof(GVecD) == 16, "layouts");

extern "C" __attribute__((visibility("default"))) int mvx_depan_analyse_host(const mvx_depan_analyse *h, int n, const void *const *blobs, const void *const *masks,
        ptrdiff_t mask_pitch, const int32_t *top_field, mvx_depan_motion *out) {
    const DepanAnalyseParams &P = h->P;
    const int nb = P.nBlkX * P.nBlkY;
    std::vector<DepanGather> rec(nb);
    std::vector<int> maskv(nb);
    for (int f = 0; f < n; f++) {
        const unsigned char *m = P.hasMask && masks ? (const unsigned char *)masks[f] : nullptr;
        if (P.hasMask && !m) { mvx_set_error("mvx_depan_analyse_host: the filter was created with a mask clip: every frame needs its mask plane"); return MVX_E_ARG; }
        const bool usable = depan_gather_host(P, (const unsigned char *)blobs[f], m, mask_pitch, rec.data(), maskv.data());
        depan_estimate(P, usable, rec.data(), maskv.data(), top_field ? top_field[f] : 0, (DepanMotion *)&out[f]);
    }
    return MVX_OK;
}

extern "C" __attribute__((visibility("default"))) int mvx_depan_analyse_frames(mvx_depan_analyse *h, int n, const void *const *blobs, const void *const *masks,
        ptrdiff_t mask_pitch, const int32_t *top_field, mvx_depan_motion *out, void *stream) {
    if (n <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    const DepanAnalyseParams &P = h->P;
    const int nb = P.nBlkX * P.nBlkY;
    const size_t stride = (16 + (size_t)nb * 20 + 15) / 16 * 16;
    std::vector<DGJob> hj(n);
    for (int f = 0; f < n; f++) {
        hj[f].blob = (const unsigned char *)blobs[f];
        hj[f].mask = P.hasMask && masks ? (const unsigned char *)masks[f] : nullptr;
        if (P.hasMask && !hj[f].mask) { mvx_set_error("mvx_depan_analyse_frames: the filter was created with a mask clip: every frame needs its mask plane"); return MVX_E_ARG; }
    }
    std::vector<unsigned char> host(stride * n);
    {
        CallGuard::Scope scope(h->guard, st);
        HIP_CHECK(h->dJobs.reserve(n));
        HIP_CHECK(h->dStaging.reserve(stride * n));
        HIP_CHECK(hipMemcpyAsync(h->dJobs.p, hj.data(), sizeof(DGJob) * n, hipMemcpyHostToDevice, st));
        DGParams G = { nb, P.nBlkX, P.nLvCount, P.stepX, P.stepY, P.nBlkSizeX / 2, P.nBlkSizeY / 2, P.width, P.height, P.thscd1, P.thscd2, (long long)mask_pitch, (long long)stride };
        hipLaunchKernelGGL(depan_gather_kernel, dim3((unsigned)n), dim3(256), 0, st, G, h->dJobs.p, h->dStaging.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(host.data(), h->dStaging.p, stride * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    for (int f = 0; f < n; f++) {
        const unsigned char *s = host.data() + stride * f;
        int verdict; memcpy(&verdict, s, 4);
        depan_estimate(P, verdict != 0, (const DepanGather *)(s + 16), (const int *)(s + 16 + (size_t)nb * 16), top_field ? top_field[f] : 0, (DepanMotion *)&out[f]);
    }
    return MVX_OK;
}
