// mvx_depan_stab.hip -- DepanStabilise on gfx950 (MVDepan.cpp:2884-4208).
//
// The smoothing of the global motion is host arithmetic (mvx_depan_stab_host.h): serial float recursions over the frames of a window, a few
// hundred operations per output frame.  What runs on the GPU is the painting.  The reference writes one destination up to three times --
// fillBorderPrev, fillBorderNext, compensateFrame (:3679-3693) -- and here one thread per output sample selects among the up-to-three
// sources (mvx_depan_stab_sample.h) and stores once:
//   depan_stab_chain_kernel : the checkpoints of the rotation form of nearest and bilinear (dc_chain_row of mvx_depan_sample.h) for every
//                             source that needs them: one flat table of DS_SOURCES records per plane, one thread per row.
//   depan_stab_kernel       : all planes of all jobs in one launch (blockIdx.z = job * planes + plane), as depan_plane_kernel of mvx_depan.hip.
// A sample inside the current frame takes exactly DepanCompensate's path.
#include <math.h>
#include "mvx_fps_shared.h"
#include "mvx_depan_stab_host.h"
#include "mvx_depan_stab_sample.h"

__global__ __launch_bounds__(64) void depan_stab_chain_kernel(const DCPlane *sources) {
    const DCPlane &P = sources[blockIdx.x];   // up to 16384 jobs x 3 planes x 3 sources: more than a grid's y extent holds
    const int h = blockIdx.y * 64 + threadIdx.x;
    if (P.src && P.cls == 2 && P.chain && h < P.H) dc_chain_row(P, h);
}

template <typename T, int SUB>
__global__ __launch_bounds__(256) void depan_stab_kernel(const DCPlane *sources, DCCommon C) {
    const DCPlane *S = sources + (size_t)blockIdx.z * DS_SOURCES;
    const int row = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    if (row >= S[DS_CUR].W || h >= S[DS_CUR].H) return;
    const int v = ds_sample<T, SUB>(S, C, h, row);
    ((T *)(S[DS_CUR].dst + (long long)h * S[DS_CUR].dpitch))[row] = (T)v;
}

struct mvx_depan_stabilise {
    CallGuard guard;
    mvx_depan_stabilise_info info;
    DepanStabParams P;
    int ssw, ssh;
    long long spitch[3], dpitch[3];
    DevBuf<DCPlane> dSources;
    DevBuf<float> dChain;
};

static float ds_arg(double v, float dflt) { return v == (double)MVX_UNSET ? dflt : (float)v; }
static int ds_arg(int32_t v, int dflt) { return v == MVX_UNSET ? dflt : v; }

// MVDepan.cpp:3909-4163 depanStabiliseCreate
extern "C" __attribute__((visibility("default"))) int mvx_depan_stabilise_create(const mvx_depan_stabilise_args *a, const mvx_depan_clip *clip, int num_frames, int data_frames,
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
    if (clip->bits > 16 || clip->bits < 8 || clip->subsampling_w > 1 || clip->subsampling_h > 1 || clip->subsampling_w < 0 || clip->subsampling_h < 0 ||
        (clip->subsampling_w == 0 && clip->subsampling_h == 1))
        MVX_FAIL("DepanStabilise: clip must have constant format and dimensions, integer sample type, bit depth up to 16, and it must be Gray, 420, 422, or 444, and not RGB.");
    if (fps_num == 0 || fps_den == 0) MVX_FAIL("DepanStabilise: clip must have known frame rate.");
    if (num_frames > data_frames) MVX_FAIL("DepanStabilise: data must have at least as many frames as clip.");
    // the library's own checks (divergences 3 and 4 of DepanCompensate, 3 and 4 of DepanStabilise in mvtools_amd.h)
    const int ssw = clip->gray ? 0 : clip->subsampling_w, ssh = clip->gray ? 0 : clip->subsampling_h;
    if (clip->width < (2 << ssw) || clip->height < (2 << ssh) || clip->width > 32767 || clip->height > 32767)
        MVX_FAIL("DepanStabilise: every plane must be at least 2 samples wide and 2 high, and the frame at most 32767 x 32767.");
    const int np = clip->gray ? 1 : 3, bps = clip->bits > 8 ? 2 : 1;
    for (int p = 0; p < np; p++)
        if (src_pitch[p] % bps || dst_pitch[p] % bps || src_pitch[p] < (clip->width >> (p ? ssw : 0)) * bps || dst_pitch[p] < (clip->width >> (p ? ssw : 0)) * bps)
            MVX_FAIL("DepanStabilise: pitches must hold a row of their plane and be multiples of the sample size.");
    if (num_frames < 1) MVX_FAIL("DepanStabilise: clip must have at least one frame.");
    if (fps_num < 0 || fps_den < 0 || !((float)fps_num / fps_den / (4 * P.cutoff) < 1048576.0f))
        MVX_FAIL("DepanStabilise: the frame rate must be positive, and fps / (4 * cutoff) below 1048576.");
    if (!(P.tzoom >= 0.0f)) MVX_FAIL("DepanStabilise: tzoom must not be negative.");

    P.width = clip->width; P.height = clip->height; P.num_frames = num_frames;
    depan_stab_init(&P, fps_num, fps_den);
    mvx_depan_stabilise *h = new mvx_depan_stabilise();
    h->P = P; h->ssw = ssw; h->ssh = ssh;
    mvx_depan_stabilise_info &I = h->info;
    memset(&I, 0, sizeof(I));
    I.width = clip->width; I.height = clip->height; I.bits = clip->bits; I.num_planes = np; I.subsampling_w = ssw; I.subsampling_h = ssh;
    I.subpixel = P.subpixel; I.mirror = P.mirror; I.pixel_max = (1 << clip->bits) - 1;
    I.method = P.method; I.prev = P.prev; I.next = P.next; I.nfields = P.nfields;
    I.radius = P.radius; I.wint_size = P.wintsize; I.winrz_size = P.winrzsize; I.winfz_size = P.winfzsize;
    for (int p = 0; p < 3; p++) {
        I.plane_width[p] = clip->width >> (p ? ssw : 0); I.plane_height[p] = clip->height >> (p ? ssh : 0);
        I.border[p] = p ? 1 << (clip->bits - 1) : 0;                              // :3362-3363, :3424
        I.blur[p] = p && ssw == 1 ? P.blur / 2 : P.blur;                          // :3371,3377
        h->spitch[p] = p < np ? src_pitch[p] : 0; h->dpitch[p] = p < np ? dst_pitch[p] : 0;
    }
    I.fps = P.fps; I.freqnative = P.freqnative; I.initzoom = P.initzoom; I.zoommax = P.zoommax; I.xcenter = P.xcenter; I.ycenter = P.ycenter;
    I.nonlinfactor[0] = P.nonlinfactor.dxc; I.nonlinfactor[1] = P.nonlinfactor.dxx; I.nonlinfactor[2] = P.nonlinfactor.dxy;
    I.nonlinfactor[3] = P.nonlinfactor.dyc; I.nonlinfactor[4] = P.nonlinfactor.dyx; I.nonlinfactor[5] = P.nonlinfactor.dyy;
    *out = h;
    return MVX_OK;
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

template <typename T> static void ds_launch(int sub, dim3 grid, hipStream_t st, const DCPlane *sources, DCCommon C) {
    if (sub == 0) hipLaunchKernelGGL((depan_stab_kernel<T, 0>), grid, dim3(256), 0, st, sources, C);
    else if (sub == 1) hipLaunchKernelGGL((depan_stab_kernel<T, 1>), grid, dim3(256), 0, st, sources, C);
    else hipLaunchKernelGGL((depan_stab_kernel<T, 2>), grid, dim3(256), 0, st, sources, C);
}

extern "C" __attribute__((visibility("default"))) int mvx_depan_stabilise_frames(mvx_depan_stabilise *h, int nframes, const mvx_depan_stabilise_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    if (nframes > 16384) { mvx_set_error("mvx_depan_stabilise_frames: at most 16384 jobs per call"); return MVX_E_ARG; }
    hipStream_t st = (hipStream_t)stream;
    CallGuard::Scope scope(h->guard, st);
    const mvx_depan_stabilise_info &I = h->info;
    const int np = I.num_planes;
    std::vector<DCPlane> hp((size_t)nframes * np * DS_SOURCES);
    size_t chain = 0;
    int maxW = 0, maxH = 0;
    for (int f = 0; f < nframes; f++) {
        const mvx_depan_stabilise_job &J = jobs[f];
        const bool use[DS_SOURCES] = { true, J.plan.next.used != 0, J.plan.prev.used != 0 };
        const float *trs[DS_SOURCES] = { J.plan.tr, J.plan.next.tr, J.plan.prev.tr };
        for (int p = 0; p < np; p++) {
            DCPlane *S = &hp[((size_t)f * np + p) * DS_SOURCES];
            const void *srcs[DS_SOURCES] = { J.cur[p], J.next[p], J.prev[p] };
            memset(S, 0, sizeof(DCPlane) * DS_SOURCES);
            if (!J.dst[p]) { mvx_set_error("mvx_depan_stabilise_frames: every plane needs dst"); return MVX_E_ARG; }
            for (int s = 0; s < DS_SOURCES; s++) {
                if (!use[s]) continue;
                DCPlane &P = S[s];
                P.src = (const unsigned char *)srcs[s]; P.dst = (unsigned char *)J.dst[p];
                if (!P.src) { mvx_set_error("mvx_depan_stabilise_frames: every plane needs the current frame and each source its plan uses"); return MVX_E_ARG; }
                P.spitch = h->spitch[p]; P.dpitch = h->dpitch[p];
                P.W = I.plane_width[p]; P.H = I.plane_height[p];
                P.blur = I.blur[p];
                ds_plane_transform(h->ssw, h->ssh, p, trs[s], &P);
                P.segs = (P.W + DC_SEG - 1) / DC_SEG;
                // the fill passes are nearest whatever subpixel is
                if (P.cls == 2 && (s != DS_CUR || I.subpixel < 2)) { P.chain = (float *)(uintptr_t)(chain + 1); chain += (size_t)P.H * P.segs * 2; } // offset + 1 until the buffer is known
            }
            ds_borders(S, I.border[p]);
            maxW = std::max(maxW, S[DS_CUR].W); maxH = std::max(maxH, S[DS_CUR].H);
        }
    }
    if (chain) HIP_CHECK(h->dChain.reserve(chain));
    for (DCPlane &P : hp) if (P.chain) P.chain = h->dChain.p + ((uintptr_t)P.chain - 1);
    HIP_CHECK(h->dSources.reserve(hp.size()));
    HIP_CHECK(hipMemcpyAsync(h->dSources.p, hp.data(), sizeof(DCPlane) * hp.size(), hipMemcpyHostToDevice, st));
    if (chain) hipLaunchKernelGGL(depan_stab_chain_kernel, dim3((unsigned)hp.size(), (unsigned)((maxH + 63) / 64)), dim3(64), 0, st, h->dSources.p);
    const DCCommon C = { I.mirror, I.pixel_max, np };
    const dim3 grid((unsigned)((maxW + 255) / 256), (unsigned)maxH, (unsigned)(hp.size() / DS_SOURCES));
    if (I.bits > 8) ds_launch<unsigned short>(I.subpixel, grid, st, h->dSources.p, C);
    else ds_launch<unsigned char>(I.subpixel, grid, st, h->dSources.p, C);
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}
