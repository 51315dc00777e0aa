// mvx_depan_warp.hip -- DepanCompensate (MVDepan.cpp:1509-2881) and DepanStabilise (:2884-4208) on gfx950: one warp engine for both.
//
// DepanCompensate warps every plane of a frame by a six-coefficient transform, xsrc = dxc + dxx * x + dxy * y, ysrc = dyc + dyx * x + dyy * y,
// with one of three interpolators (compensate_plane_nearest / _bilinear / _bicubic, :1626-2585), each of which has three forms chosen by
// float comparisons on the coefficients: translation only, zoom without rotation, rotation.  DepanStabilise smooths the global motion on the
// host (mvx_depan_stab_host.h: serial float recursions over the frames of a window, a few hundred operations per output frame) and paints:
// the reference writes one destination up to three times -- fillBorderPrev, fillBorderNext, compensateFrame (:3679-3693) -- and here one
// thread per output sample selects among the up-to-three sources and stores once.  Both filters put one DCPlane record per (plane, source)
// into a flat table, NSRC records per plane (1, or DS_SOURCES), and run:
//   depan_chain_kernel : rotation form of nearest and bilinear only.  The reference walks a row by xsrc += dxx, ysrc += dyx in float, so
//                        column k holds k sequential roundings.  One thread per row repeats that walk and stores the pair every DC_SEG
//                        columns into scratch of the filter object, for every record that needs it.
//   depan_warp_kernel  : one thread per output sample, all planes of all jobs in one launch (blockIdx.z = job * planes + plane).  It takes at
//                        most DC_SEG - 1 additions from its checkpoint, or computes the position as the reference's form does, then restates
//                        that form's branches: mirror bits, blur runs, the edge rows, bicubic's double near-edge rows and its clamp.
// Where the reference's own index leaves its row (the unchecked mirror column and the blur runs) the border value is written; see the
// divergences in mvtools_amd.h.  Positions that are NaN or not inside (-2^30, 2^30) -- where the reference's float -> int conversion is
// undefined or its mirror arithmetic overflows -- give the border value too.  A sample of DepanStabilise inside the current frame takes
// exactly DepanCompensate's path.
#include <math.h>
#include "mvx_fps_shared.h"
#include "mvx_depan_host.h"
#include "mvx_depan_stab_host.h"
#include "mvx_depan_sample.h"
#include "mvx_depan_sample_float.h"

__global__ __launch_bounds__(64) void depan_chain_kernel(const DCPlane *planes) {
    const DCPlane &P = planes[blockIdx.x];   // up to 16384 jobs x 3 planes x 3 sources: more than a grid's y extent holds
    const int h = blockIdx.y * 64 + threadIdx.x;
    if (P.src && P.cls == 2 && P.chain && h < P.H) dc_chain_row(P, h);
}

template <typename T, int SUB, int NSRC>
__global__ __launch_bounds__(256) void depan_warp_kernel(const DCPlane *planes, DCCommon C) {
    const DCPlane *S = planes + (size_t)blockIdx.z * NSRC;
    const int row = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    if (row >= S[DS_CUR].W || h >= S[DS_CUR].H) return;
    if constexpr (sizeof(T) == 4) dcf_store<SUB, NSRC>(S, C, h, row);   // a float clip: mvx_depan_sample_float.h
    else dc_store<T, SUB, NSRC>(S, C, h, row);
}

// ------------------------------------------------------------------------------------------------ the engine both filters derive from

struct DepanWarp {
    CallGuard guard;
    DCClip G;
    DevBuf<DCPlane> dPlanes;
    DevBuf<float> dChain;

    // the host table of one call: NSRC records per plane of every job, zeroed (an unused source has src == nullptr)
    struct Table {
        std::vector<DCPlane> rec;
        size_t chain = 0;
        explicit Table(size_t n) : rec(n) { memset(rec.data(), 0, sizeof(DCPlane) * n); }
    };
    void add(Table &T, size_t i, int p, const void *src, void *dst, const float *tr, bool fill) const {
        const size_t n = dc_fill(G, p, src, dst, tr, fill, &T.rec[i]);
        if (n) { T.rec[i].chain = (float *)(uintptr_t)(T.chain + 1); T.chain += n; } // offset + 1 until the buffer is known
    }

    template <typename T, int NSRC> void dispatch(dim3 grid, hipStream_t st, DCCommon C) {
        if (G.subpixel == 0) hipLaunchKernelGGL((depan_warp_kernel<T, 0, NSRC>), grid, dim3(256), 0, st, dPlanes.p, C);
        else if (G.subpixel == 1) hipLaunchKernelGGL((depan_warp_kernel<T, 1, NSRC>), grid, dim3(256), 0, st, dPlanes.p, C);
        else hipLaunchKernelGGL((depan_warp_kernel<T, 2, NSRC>), grid, dim3(256), 0, st, dPlanes.p, C);
    }
    template <int NSRC> int launch(Table &T, void *stream) {
        hipStream_t st = (hipStream_t)stream;
        CallGuard::Scope scope(guard, st);
        if (T.chain) HIP_CHECK(dChain.reserve(T.chain));
        for (DCPlane &P : T.rec) if (P.chain) P.chain = dChain.p + ((uintptr_t)P.chain - 1);
        HIP_CHECK(dPlanes.reserve(T.rec.size()));
        HIP_CHECK(hipMemcpyAsync(dPlanes.p, T.rec.data(), sizeof(DCPlane) * T.rec.size(), hipMemcpyHostToDevice, st));
        if (T.chain) hipLaunchKernelGGL(depan_chain_kernel, dim3((unsigned)T.rec.size(), (unsigned)((G.H[0] + 63) / 64)), dim3(64), 0, st, dPlanes.p);
        const DCCommon C = { G.mirror, G.pixel_max, G.np };
        const dim3 grid((unsigned)((G.W[0] + 255) / 256), (unsigned)G.H[0], (unsigned)(T.rec.size() / NSRC)); // luma is the largest plane
        if (G.bits == 32) dispatch<float, NSRC>(grid, st, C);
        else if (G.bits > 8) dispatch<unsigned short, NSRC>(grid, st, C);
        else dispatch<unsigned char, NSRC>(grid, st, C);
        HIP_CHECK(hipGetLastError());
        return MVX_OK;
    }
};

// The checks and fields the two creation functions share, at their place in each filter's order of messages: the reference's format
// message; `refusal`, the filter's own message that the reference places next (nullptr: none applies); then the library's own checks
// (divergences 3 and 4 of DepanCompensate in mvtools_amd.h).  Info: mvx_depan_compensate_info or mvx_depan_stabilise_info, zeroed but for
// the shared fields.  is_float: the *_create_float entries -- a 32-bit float clip; where the format message sits, one more for a clip that
// is not 32-bit; samples of 4 bytes; info.pixel_max and info.border[] are 0 (the border is 0.0f luma and 0.5f chroma: G->border holds it in
// halves for mvx_depan_sample_float.h).
template <typename Info> static int depan_warp_create(const char *name, bool is_float, const mvx_depan_clip *clip, const char *refusal, const ptrdiff_t src_pitch[3],
        const ptrdiff_t dst_pitch[3], int subpixel, int mirror, int blur, DCClip *G, Info *I, char *err) {
    if (is_float && clip->bits != 32) MVX_FAIL("%s: the float path takes a 32-bit float clip; create an 8..16 bit clip's filter with the integer entry.", name);
    if ((!is_float && (clip->bits > 16 || clip->bits < 8)) || clip->subsampling_w > 1 || clip->subsampling_h > 1 || clip->subsampling_w < 0 || clip->subsampling_h < 0 ||
        (clip->subsampling_w == 0 && clip->subsampling_h == 1))
        MVX_FAIL("%s: clip must have constant format and dimensions, integer sample type, bit depth up to 16, and it must be Gray, 420, 422, or 444, and not RGB.", name);
    if (refusal) MVX_FAIL("%s", refusal);
    const int ssw = clip->gray ? 0 : clip->subsampling_w, ssh = clip->gray ? 0 : clip->subsampling_h;
    if (clip->width < (2 << ssw) || clip->height < (2 << ssh) || clip->width > 32767 || clip->height > 32767)
        MVX_FAIL("%s: every plane must be at least 2 samples wide and 2 high, and the frame at most 32767 x 32767.", name);
    const int np = clip->gray ? 1 : 3, bps = is_float ? 4 : clip->bits > 8 ? 2 : 1;
    for (int p = 0; p < np; p++)
        if (src_pitch[p] % bps || dst_pitch[p] % bps || src_pitch[p] < (clip->width >> (p ? ssw : 0)) * bps || dst_pitch[p] < (clip->width >> (p ? ssw : 0)) * bps)
            MVX_FAIL("%s: pitches must hold a row of their plane and be multiples of the sample size.", name);
    memset(G, 0, sizeof(*G));
    memset(I, 0, sizeof(*I));
    I->width = clip->width; I->height = clip->height;
    I->bits = G->bits = clip->bits; I->num_planes = G->np = np; I->subsampling_w = G->ssw = ssw; I->subsampling_h = G->ssh = ssh;
    I->subpixel = G->subpixel = subpixel; I->mirror = G->mirror = mirror; I->pixel_max = G->pixel_max = is_float ? 0 : (1 << clip->bits) - 1;
    for (int p = 0; p < 3; p++) {
        I->plane_width[p] = G->W[p] = clip->width >> (p ? ssw : 0); I->plane_height[p] = G->H[p] = clip->height >> (p ? ssh : 0);
        I->border[p] = is_float ? 0 : p ? 1 << (clip->bits - 1) : 0;             // :2683 / :3362-3363, :3424
        G->border[p] = is_float ? (p ? 1 : 0) : I->border[p];
        I->blur[p] = G->blur[p] = p && ssw == 1 ? blur / 2 : blur;                // :2684,2692,2698 / :3371,3377
        G->spitch[p] = p < np ? src_pitch[p] : 0; G->dpitch[p] = p < np ? dst_pitch[p] : 0;
    }
    return MVX_OK;
}

// ------------------------------------------------------------------------------------------------ DepanCompensate

struct mvx_depan_compensate : DepanWarp {
    mvx_depan_compensate_info info;
    float offset, pixaspect, xcenter, ycenter;
    int matchfields, fields, tff, tff_exists, num_frames;
};

// MVDepan.cpp:2750-2881 depanCompensateCreate
static int depan_compensate_create(bool is_float, const mvx_depan_compensate_args *a, const mvx_depan_clip *clip, int num_frames, int data_frames,
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
    DCClip G;
    mvx_depan_compensate_info I;
    if (int rc = depan_warp_create("DepanCompensate", is_float, clip, num_frames > data_frames ? "DepanCompensate: data must have at least as many frames as clip." : nullptr,
                                   src_pitch, dst_pitch, subpixel, mirror, blur, &G, &I, err)) return rc;

    mvx_depan_compensate *h = new mvx_depan_compensate();
    h->G = G;
    h->offset = offset; h->pixaspect = pixaspect; h->matchfields = matchfields; h->fields = fields; h->num_frames = num_frames;
    h->tff_exists = a->tff != MVX_UNSET; h->tff = h->tff_exists ? !!a->tff : 0;
    h->xcenter = clip->width / 2.0f; h->ycenter = clip->height / 2.0f; // :2840-2841
    I.intoffset = offset > 0.0f ? (int)ceilf(offset) : (int)floorf(offset);     // :2835-2838
    I.xcenter = h->xcenter; I.ycenter = h->ycenter; I.offset = offset; I.pixaspect = pixaspect;
    h->info = I;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) int mvx_depan_compensate_create(const mvx_depan_compensate_args *a, const mvx_depan_clip *clip, int num_frames, int data_frames,
        const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3], mvx_depan_compensate **out, char *err) {
    return depan_compensate_create(false, a, clip, num_frames, data_frames, src_pitch, dst_pitch, out, err);
}
// the same filter on a 32-bit float clip (mvx_depan_sample_float.h); no device is touched
extern "C" __attribute__((visibility("default"))) int mvx_depan_compensate_create_float(const mvx_depan_compensate_args *a, const mvx_depan_clip *clip, int num_frames, int data_frames,
        const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3], mvx_depan_compensate **out, char *err) {
    return depan_compensate_create(true, a, clip, num_frames, data_frames, src_pitch, dst_pitch, out, err);
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

extern "C" __attribute__((visibility("default"))) int mvx_depan_compensate_frames(mvx_depan_compensate *h, int nframes, const mvx_depan_compensate_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    if (nframes > 16384) { mvx_set_error("mvx_depan_compensate_frames: at most 16384 jobs per call"); return MVX_E_ARG; }
    const int np = h->G.np;
    DepanWarp::Table T((size_t)nframes * np);
    for (int f = 0; f < nframes; f++)
        for (int p = 0; p < np; p++) {
            if (!jobs[f].src[p] || !jobs[f].dst[p]) { mvx_set_error("mvx_depan_compensate_frames: every plane needs src and dst"); return MVX_E_ARG; }
            h->add(T, (size_t)f * np + p, p, jobs[f].src[p], jobs[f].dst[p], jobs[f].tr, false);
        }
    return h->launch<1>(T, stream);
}

// ------------------------------------------------------------------------------------------------ DepanStabilise

struct mvx_depan_stabilise : DepanWarp {
    mvx_depan_stabilise_info info;
    DepanStabParams P;
};

static float ds_arg(double v, float dflt) { return v == (double)MVX_UNSET ? dflt : (float)v; }
static int ds_arg(int32_t v, int dflt) { return v == MVX_UNSET ? dflt : v; }

// MVDepan.cpp:3909-4163 depanStabiliseCreate
static int depan_stabilise_create(bool is_float, const mvx_depan_stabilise_args *a, const mvx_depan_clip *clip, int num_frames, int data_frames,
        int64_t fps_num, int64_t fps_den, const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3], mvx_depan_stabilise **out, char *err) {
    MVX_CREATE_BEGIN(out);
    DepanStabParams P;
    P.cutoff = ds_arg(a->cutoff, 1.0f); P.damping = ds_arg(a->damping, 0.9f); P.initzoom = ds_arg(a->initzoom, 1.0f);
    P.addzoom = !!ds_arg(a->addzoom, 0); P.prev = ds_arg(a->prev, 0); P.next = ds_arg(a->next, 0); P.mirror = ds_arg(a->mirror, 0); P.blur = ds_arg(a->blur, 0);
    P.dxmax = ds_arg(a->dxmax, 60.0f); P.dymax = ds_arg(a->dymax, 30.0f); P.zoommax = ds_arg(a->zoommax, 1.05f); P.rotmax = ds_arg(a->rotmax, 1.0f);
    P.subpixel = ds_arg(a->subpixel, 2); P.pixaspect = ds_arg(a->pixaspect, 1.0f); P.fitlast = ds_arg(a->fitlast, 0); P.tzoom = ds_arg(a->tzoom, 3.0f);
    P.method = ds_arg(a->method, 0); P.fields = !!ds_arg(a->fields, 0);
    if (P.cutoff <= 0.0f) MVX_FAIL("DepanStabilise: cutoff must be greater than 0.");
    if (P.prev < 0) MVX_FAIL("DepanStabilise: prev must not be negative.");
    if (P.next < 0) MVX_FAIL("DepanStabilise: next must not be negative.");
    if (P.subpixel < 0 || P.subpixel > 2) MVX_FAIL("DepanStabilise: subpixel must be between 0 and 2 (inclusive).");
    if (P.pixaspect <= 0.0f) MVX_FAIL("DepanStabilise: pixaspect must be greater than 0.");
    if (P.mirror < 0 || P.mirror > 15) MVX_FAIL("DepanStabilise: mirror must be between 0 and 15 (inclusive).");
    if (P.blur < 0) MVX_FAIL("DepanStabilise: blur must not be negative.");
    if (P.method < 0 || P.method > 1) MVX_FAIL("DepanStabilise: method must be between 0 and 1 (inclusive).");
    DCClip G;
    mvx_depan_stabilise_info I;
    if (int rc = depan_warp_create("DepanStabilise", is_float, clip, fps_num == 0 || fps_den == 0 ? "DepanStabilise: clip must have known frame rate."
                                   : num_frames > data_frames ? "DepanStabilise: data must have at least as many frames as clip." : nullptr,
                                   src_pitch, dst_pitch, P.subpixel, P.mirror, P.blur, &G, &I, err)) return rc;
    // the library's own checks (divergence 3 of DepanStabilise in mvtools_amd.h)
    if (num_frames < 1) MVX_FAIL("DepanStabilise: clip must have at least one frame.");
    if (fps_num < 0 || fps_den < 0 || !((float)fps_num / fps_den / (4 * P.cutoff) < 1048576.0f))
        MVX_FAIL("DepanStabilise: the frame rate must be positive, and fps / (4 * cutoff) below 1048576.");
    if (!(P.tzoom >= 0.0f)) MVX_FAIL("DepanStabilise: tzoom must not be negative.");

    P.width = clip->width; P.height = clip->height; P.num_frames = num_frames;
    depan_stab_init(&P, fps_num, fps_den);
    mvx_depan_stabilise *h = new mvx_depan_stabilise();
    h->G = G; h->P = P;
    I.method = P.method; I.prev = P.prev; I.next = P.next; I.nfields = P.nfields;
    I.radius = P.radius; I.wint_size = P.wintsize; I.winrz_size = P.winrzsize; I.winfz_size = P.winfzsize;
    I.fps = P.fps; I.freqnative = P.freqnative; I.initzoom = P.initzoom; I.zoommax = P.zoommax; I.xcenter = P.xcenter; I.ycenter = P.ycenter;
    I.nonlinfactor[0] = P.nonlinfactor.dxc; I.nonlinfactor[1] = P.nonlinfactor.dxx; I.nonlinfactor[2] = P.nonlinfactor.dxy;
    I.nonlinfactor[3] = P.nonlinfactor.dyc; I.nonlinfactor[4] = P.nonlinfactor.dyx; I.nonlinfactor[5] = P.nonlinfactor.dyy;
    h->info = I;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) int mvx_depan_stabilise_create(const mvx_depan_stabilise_args *a, const mvx_depan_clip *clip, int num_frames, int data_frames,
        int64_t fps_num, int64_t fps_den, const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3], mvx_depan_stabilise **out, char *err) {
    return depan_stabilise_create(false, a, clip, num_frames, data_frames, fps_num, fps_den, src_pitch, dst_pitch, out, err);
}
// the same filter on a 32-bit float clip (mvx_depan_sample_float.h); no device is touched
extern "C" __attribute__((visibility("default"))) int mvx_depan_stabilise_create_float(const mvx_depan_stabilise_args *a, const mvx_depan_clip *clip, int num_frames, int data_frames,
        int64_t fps_num, int64_t fps_den, const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3], mvx_depan_stabilise **out, char *err) {
    return depan_stabilise_create(true, a, clip, num_frames, data_frames, fps_num, fps_den, src_pitch, dst_pitch, out, err);
}
extern "C" __attribute__((visibility("default"))) void mvx_depan_stabilise_destroy(mvx_depan_stabilise *h) { delete h; }
extern "C" __attribute__((visibility("default"))) void mvx_depan_stabilise_get_info(const mvx_depan_stabilise *h, mvx_depan_stabilise_info *info) { *info = h->info; }
extern "C" __attribute__((visibility("default"))) void mvx_depan_stabilise_get_windows(const mvx_depan_stabilise *h, float *wint, float *winrz, float *winfz) {
    const size_t n = (size_t)h->P.wintsize + 1;
    if (wint) memcpy(wint, h->P.wint.data(), n * sizeof(float));
    if (winrz) memcpy(winrz, h->P.winrz.data(), n * sizeof(float));
    if (winfz) memcpy(winfz, h->P.winfz.data(), n * sizeof(float));
}

extern "C" __attribute__((visibility("default"))) int mvx_depan_stabilise_window(const mvx_depan_stabilise *h, int n, int *data_first, int *data_last, int *clip_first, int *clip_last) {
    if (n < 0 || n >= h->P.num_frames) { mvx_set_error("mvx_depan_stabilise_window: frame %d is outside the clip", n); return MVX_E_ARG; }
    int a, b, c, d;
    depan_stab_window(&h->P, n, &a, &b, &c, &d);
    if (data_first) *data_first = a;
    if (data_last) *data_last = b;
    if (clip_first) *clip_first = c;
    if (clip_last) *clip_last = d;
    return MVX_OK;
}

static_assert(sizeof(DepanStabPlan) == sizeof(mvx_depan_stabilise_frame_plan) && sizeof(DepanStabSource) == sizeof(mvx_depan_stabilise_source), "layouts");

extern "C" __attribute__((visibility("default"))) int mvx_depan_stabilise_plan(const mvx_depan_stabilise *h, int n, const float *motions, mvx_depan_stabilise_frame_plan *plan, char *err) {
    MVX_ERR_BEGIN();
    if (n < 0 || n >= h->P.num_frames) MVX_FAIL("mvx_depan_stabilise_plan: frame %d is outside the clip", n);
    if (!motions || !plan) MVX_FAIL("mvx_depan_stabilise_plan: motions and plan are required");
    depan_stab_plan(&h->P, n, motions, (DepanStabPlan *)plan);
    return MVX_OK;
}

extern "C" __attribute__((visibility("default"))) int mvx_depan_stabilise_frames(mvx_depan_stabilise *h, int nframes, const mvx_depan_stabilise_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    if (nframes > 16384) { mvx_set_error("mvx_depan_stabilise_frames: at most 16384 jobs per call"); return MVX_E_ARG; }
    const int np = h->G.np;
    DepanWarp::Table T((size_t)nframes * np * DS_SOURCES);
    for (int f = 0; f < nframes; f++) {
        const mvx_depan_stabilise_job &J = jobs[f];
        const bool use[DS_SOURCES] = { true, J.plan.next.used != 0, J.plan.prev.used != 0 };
        const float *trs[DS_SOURCES] = { J.plan.tr, J.plan.next.tr, J.plan.prev.tr };
        for (int p = 0; p < np; p++) {
            const size_t i = ((size_t)f * np + p) * DS_SOURCES;
            const void *srcs[DS_SOURCES] = { J.cur[p], J.next[p], J.prev[p] };
            if (!J.dst[p]) { mvx_set_error("mvx_depan_stabilise_frames: every plane needs dst"); return MVX_E_ARG; }
            for (int s = 0; s < DS_SOURCES; s++) {
                if (!use[s]) continue;
                if (!srcs[s]) { mvx_set_error("mvx_depan_stabilise_frames: every plane needs the current frame and each source its plan uses"); return MVX_E_ARG; }
                h->add(T, i + s, p, srcs[s], J.dst[p], trs[s], s != DS_CUR);
            }
            ds_borders(&T.rec[i], h->G.border[p]);
        }
    }
    return h->launch<DS_SOURCES>(T, stream);
}
