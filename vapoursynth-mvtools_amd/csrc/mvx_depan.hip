// mvx_depan.hip -- DepanCompensate and DepanAnalyse on gfx950 (MVDepan.cpp:41-615 DepanAnalyse, :1509-2881 DepanCompensate).
//
// DepanCompensate warps every plane of a frame by a six-coefficient transform, xsrc = dxc + dxx * x + dxy * y, ysrc = dyc + dyx * x + dyy * y,
// with one of three interpolators (compensate_plane_nearest / _bilinear / _bicubic, :1626-2585), each of which has three forms chosen by
// float comparisons on the coefficients: translation only, zoom without rotation, rotation.  Here:
//   depan_chain_kernel : rotation form of nearest and bilinear only.  The reference walks a row by xsrc += dxx, ysrc += dyx in float, so
//                        column k holds k sequential roundings.  One thread per row repeats that walk and stores the pair every DC_SEG
//                        columns into scratch of the filter object.
//   depan_plane_kernel : one thread per output sample, all planes of all jobs in one launch (blockIdx.z = job * planes + plane).  It takes at
//                        most DC_SEG - 1 additions from its checkpoint, or computes the position as the reference's form does, then restates
//                        that form's branches: mirror bits, blur runs, the edge rows, bicubic's double near-edge rows and its clamp.
// Where the reference's own index leaves its row (the unchecked mirror column and the blur runs) the border value is written; see the
// divergences in mvtools_amd.h.  Positions that are NaN or not inside (-2^30, 2^30) -- where the reference's float -> int conversion is
// undefined or its mirror arithmetic overflows -- give the border value too.
//
// DepanAnalyse: depan_gather_kernel writes the verdict of fgopIsUsable, the level-0 records and the mask byte under every block centre of all
// jobs into a staging buffer; the estimator (mvx_depan_host.h) runs on the host, in block order, because every one of its sums is a
// serial float chain.
#include <math.h>
#include "mvx_fps_shared.h"
#include "mvx_depan_host.h"
#include "mvx_depan_sample.h"

__global__ __launch_bounds__(64) void depan_chain_kernel(const DCPlane *planes) {
    const DCPlane &P = planes[blockIdx.y];
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (P.cls == 2 && P.chain && h < P.H) dc_chain_row(P, h);
}

template <typename T, int SUB>
__global__ __launch_bounds__(256) void depan_plane_kernel(const DCPlane *planes, DCCommon C) {
    const DCPlane &P = planes[blockIdx.z];
    const int row = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    if (row >= P.W || h >= P.H) return;
    const int v = SUB == 0 ? dc_nearest<T>(P, C, h, row) : SUB == 1 ? dc_bilinear<T>(P, C, h, row) : dc_bicubic<T>(P, C, h, row);
    ((T *)(P.dst + (long long)h * P.dpitch))[row] = (T)v;
}

// ------------------------------------------------------------------------------------------------ DepanCompensate, host object

struct mvx_depan_compensate {
    CallGuard guard;
    mvx_depan_compensate_info info;
    float offset, pixaspect, xcenter, ycenter;
    int matchfields, fields, tff, tff_exists, num_frames;
    int ssw, ssh;
    long long spitch[3], dpitch[3];
    DevBuf<DCPlane> dPlanes;
    DevBuf<float> dChain;
};

// MVDepan.cpp:2750-2881 depanCompensateCreate
extern "C" __attribute__((visibility("default"))) int mvx_depan_compensate_create(const mvx_depan_compensate_args *a, const mvx_depan_clip *clip, int num_frames, int data_frames,
        const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3], mvx_depan_compensate **out, char *err) {
    MVX_CREATE_BEGIN(out);
    const float offset = (float)a->offset, pixaspect = (float)a->pixaspect;
    const int subpixel = a->subpixel == MVX_UNSET ? 2 : a->subpixel;
    const int matchfields = a->matchfields == MVX_UNSET ? 1 : !!a->matchfields;
    const int mirror = a->mirror == MVX_UNSET ? 0 : a->mirror, blur = a->blur == MVX_UNSET ? 0 : a->blur;
    const int fields = a->fields == MVX_UNSET ? 0 : !!a->fields;
    if (offset < -10.0f || offset > 10.0f) MVX_FAIL("DepanCompensate: offset must be between -10.0 and 10.0 (inclusive).");
    if (subpixel < 0 || subpixel > 2) MVX_FAIL("DepanCompensate: subpixel must be between 0 and 2 (inclusive).");
    if (pixaspect <= 0.0f) MVX_FAIL("DepanCompensate: pixaspect must be greater than 0.");
    if (mirror < 0 || mirror > 15) MVX_FAIL("DepanCompensate: mirror must be between 0 and 15 (inclusive).");
    if (blur < 0) MVX_FAIL("DepanCompensate: blur must not be negative.");
    if (clip->bits > 16 || clip->bits < 8 || clip->subsampling_w > 1 || clip->subsampling_h > 1 || clip->subsampling_w < 0 || clip->subsampling_h < 0 ||
        (clip->subsampling_w == 0 && clip->subsampling_h == 1))
        MVX_FAIL("DepanCompensate: clip must have constant format and dimensions, integer sample type, bit depth up to 16, and it must be Gray, 420, 422, or 444, and not RGB.");
    if (num_frames > data_frames) MVX_FAIL("DepanCompensate: data must have at least as many frames as clip.");
    // the library's own checks (divergences 3 and 4 of mvtools_amd.h)
    const int ssw = clip->gray ? 0 : clip->subsampling_w, ssh = clip->gray ? 0 : clip->subsampling_h;
    if (clip->width < (2 << ssw) || clip->height < (2 << ssh) || clip->width > 32767 || clip->height > 32767)
        MVX_FAIL("DepanCompensate: every plane must be at least 2 samples wide and 2 high, and the frame at most 32767 x 32767.");
    const int np = clip->gray ? 1 : 3, bps = clip->bits > 8 ? 2 : 1;
    for (int p = 0; p < np; p++)
        if (src_pitch[p] % bps || dst_pitch[p] % bps || src_pitch[p] < (clip->width >> (p ? ssw : 0)) * bps || dst_pitch[p] < (clip->width >> (p ? ssw : 0)) * bps)
            MVX_FAIL("DepanCompensate: pitches must hold a row of their plane and be multiples of the sample size.");

    mvx_depan_compensate *h = new mvx_depan_compensate();
    h->offset = offset; h->pixaspect = pixaspect; h->matchfields = matchfields; h->fields = fields; h->num_frames = num_frames;
    h->tff_exists = a->tff != MVX_UNSET; h->tff = h->tff_exists ? !!a->tff : 0;
    h->ssw = ssw; h->ssh = ssh;
    h->xcenter = clip->width / 2.0f; h->ycenter = clip->height / 2.0f; // :2840-2841
    mvx_depan_compensate_info &I = h->info;
    memset(&I, 0, sizeof(I));
    I.width = clip->width; I.height = clip->height; I.bits = clip->bits; I.num_planes = np; I.subsampling_w = ssw; I.subsampling_h = ssh;
    I.intoffset = offset > 0.0f ? (int)ceilf(offset) : (int)floorf(offset);     // :2835-2838
    I.subpixel = subpixel; I.mirror = mirror; I.pixel_max = (1 << clip->bits) - 1;
    for (int p = 0; p < 3; p++) {
        I.plane_width[p] = clip->width >> (p ? ssw : 0); I.plane_height[p] = clip->height >> (p ? ssh : 0);
        I.border[p] = p ? 1 << (clip->bits - 1) : 0;                              // :2683
        I.blur[p] = p && ssw == 1 ? blur / 2 : blur;                              // :2684,2692,2698
        h->spitch[p] = p < np ? src_pitch[p] : 0; h->dpitch[p] = p < np ? dst_pitch[p] : 0;
    }
    I.xcenter = h->xcenter; I.ycenter = h->ycenter; I.offset = offset; I.pixaspect = pixaspect;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) void mvx_depan_compensate_destroy(mvx_depan_compensate *h) { delete h; }
extern "C" __attribute__((visibility("default"))) void mvx_depan_compensate_get_info(const mvx_depan_compensate *h, mvx_depan_compensate_info *info) { *info = h->info; }

// MVDepan.cpp:2594-2602,2611-2623: 1 and the frames to read, or 0: the caller returns clip frame ndest itself
extern "C" __attribute__((visibility("default"))) int mvx_depan_compensate_map(const mvx_depan_compensate *h, int ndest, int *nsrc, int *start, int *end) {
    const int n = ndest - h->info.intoffset;
    const bool pass = h->info.intoffset == 0 || n < 0 || n > h->num_frames - 1;
    if (nsrc) *nsrc = pass ? ndest : n;
    if (start) *start = pass ? ndest : std::min(n, ndest);
    if (end) *end = pass ? ndest : std::max(n, ndest);
    return pass ? 0 : 1;
}

// MVDepan.cpp:2616-2675, and transform2motion of :2718-2719
extern "C" __attribute__((visibility("default"))) int mvx_depan_motion_to_transform(const mvx_depan_compensate *h, int count, const float *motions, int ndest, int top_field,
        float trsum[6], float motion[4], char *err) {
    MVX_ERR_BEGIN();
    float halfline = 0.0f;
    if (h->fields && h->matchfields) {
        if (top_field == MVX_UNSET && !h->tff_exists) MVX_FAIL("DepanCompensate: _Field property not found in input frame. Therefore, you must pass tff argument.");
        int top = top_field == MVX_UNSET ? 0 : !!top_field;
        if (h->tff_exists) top = h->tff ^ (ndest % 2);
        halfline = top ? -0.5f : 0.5f;
    }
    DepanTransform t;
    depan_compensate_transform(motions, count, h->offset, h->info.intoffset, h->fields, h->pixaspect, h->xcenter, h->ycenter, halfline, &t, motion);
    memcpy(trsum, &t, sizeof(t));
    return MVX_OK;
}

// the plane's transform, MVDepan.cpp:2687-2700, and its form, the comparisons of :1666,1733 (the same in all three interpolators)
static void dc_plane_transform(const mvx_depan_compensate *h, int p, const float *tr, DCPlane *P) {
    DepanTransform t;
    memcpy(&t, tr, sizeof(t));
    if (p && h->ssw == 1 && h->ssh == 1) { t.dxc /= 2; t.dyc /= 2; }
    else if (p && h->ssw == 1 && h->ssh == 0) { t.dxc /= 2; t.dxy /= 2; t.dyx *= 2; }
    P->dxc = t.dxc; P->dxx = t.dxx; P->dxy = t.dxy; P->dyc = t.dyc; P->dyx = t.dyx; P->dyy = t.dyy;
    P->cls = (t.dxy == 0.0f && t.dyx == 0.0f && t.dxx == 1.0f && t.dyy == 1.0f) ? 0 : (t.dxy == 0.0f && t.dyx == 0.0f) ? 1 : 2;
}

template <typename T> static void dc_launch(int sub, dim3 grid, hipStream_t st, const DCPlane *planes, DCCommon C) {
    if (sub == 0) hipLaunchKernelGGL((depan_plane_kernel<T, 0>), grid, dim3(256), 0, st, planes, C);
    else if (sub == 1) hipLaunchKernelGGL((depan_plane_kernel<T, 1>), grid, dim3(256), 0, st, planes, C);
    else hipLaunchKernelGGL((depan_plane_kernel<T, 2>), grid, dim3(256), 0, st, planes, C);
}

extern "C" __attribute__((visibility("default"))) int mvx_depan_compensate_frames(mvx_depan_compensate *h, int nframes, const mvx_depan_compensate_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    if (nframes > 16384) { mvx_set_error("mvx_depan_compensate_frames: at most 16384 jobs per call"); return MVX_E_ARG; }
    hipStream_t st = (hipStream_t)stream;
    CallGuard::Scope scope(h->guard, st);
    const mvx_depan_compensate_info &I = h->info;
    const int np = I.num_planes;
    std::vector<DCPlane> hp((size_t)nframes * np);
    size_t chain = 0;
    int maxW = 0, maxH = 0;
    for (int f = 0; f < nframes; f++)
        for (int p = 0; p < np; p++) {
            DCPlane &P = hp[(size_t)f * np + p];
            memset(&P, 0, sizeof(P));
            P.src = (const unsigned char *)jobs[f].src[p]; P.dst = (unsigned char *)jobs[f].dst[p];
            if (!P.src || !P.dst) { mvx_set_error("mvx_depan_compensate_frames: every plane needs src and dst"); return MVX_E_ARG; }
            P.spitch = h->spitch[p]; P.dpitch = h->dpitch[p];
            P.W = I.plane_width[p]; P.H = I.plane_height[p];
            P.border = I.border[p]; P.blur = I.blur[p];
            dc_plane_transform(h, p, jobs[f].tr, &P);
            P.segs = (P.W + DC_SEG - 1) / DC_SEG;
            if (P.cls == 2 && I.subpixel < 2) { P.chain = (float *)(uintptr_t)(chain + 1); chain += (size_t)P.H * P.segs * 2; } // offset + 1 until the buffer is known
            maxW = std::max(maxW, P.W); maxH = std::max(maxH, P.H);
        }
    if (chain) HIP_CHECK(h->dChain.reserve(chain));
    for (DCPlane &P : hp) if (P.chain) P.chain = h->dChain.p + ((uintptr_t)P.chain - 1);
    HIP_CHECK(h->dPlanes.reserve(hp.size()));
    HIP_CHECK(hipMemcpyAsync(h->dPlanes.p, hp.data(), sizeof(DCPlane) * hp.size(), hipMemcpyHostToDevice, st));
    if (chain) hipLaunchKernelGGL(depan_chain_kernel, dim3((unsigned)((maxH + 63) / 64), (unsigned)hp.size()), dim3(64), 0, st, h->dPlanes.p);
    const DCCommon C = { I.mirror, I.pixel_max, np };
    const dim3 grid((unsigned)((maxW + 255) / 256), (unsigned)maxH, (unsigned)hp.size());
    if (I.bits > 8) dc_launch<unsigned short>(I.subpixel, grid, st, h->dPlanes.p, C);
    else dc_launch<unsigned char>(I.subpixel, grid, st, h->dPlanes.p, C);
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}

// ------------------------------------------------------------------------------------------------ DepanAnalyse

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
