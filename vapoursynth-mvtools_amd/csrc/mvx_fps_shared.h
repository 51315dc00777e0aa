// mvx_fps_shared.h -- what the filters that consume vectors share (the block filters through mvx_block_shared.h: mvx_degrain.hip, mvx_degrain_n.hip,
// mvx_compensate.hip, mvx_blockfps.hip; mvx_flow.hip, mvx_mask.hip).  Device side: the level-0
// vector reader, fgopIsUsable, the super-plane addressing, the wide sample loads / stores, the reference's bilinear upsizer and the occlusion
// mask of MaskFun.cpp.  Host side: the scene-change thresholds, the checks on a pair of vector clips, the frame-rate conversion, the padded
// small-field grid with its upsizer tables, the plane geometry and the launch dispatch by sample type and width.  What only the block filters
// share is in mvx_block_shared.h, on top of this.  Internal; not part of the ABI.
#pragma once
#include <algorithm>
#include <type_traits>
#include "mvx_common.h"

struct __attribute__((packed, aligned(4))) GVecD { int x, y; long long sad; };

// level-0 vectors of a MVTools_vectors blob: skip size + validity, then every coarser plane by ITS OWN size header -- the
// reference's reader does exactly this, which is what makes clips produced with divide (an extra array of half-size
// blocks after the finest estimated plane, whose geometry the level formula does not describe) readable
// pointers that come out of job tables are generic ("flat") to the compiler: loads through them are slower and each is waited for on its own
#define DG_GL __attribute__((address_space(1)))
__device__ __forceinline__ DG_GL const unsigned char *dg_gl(const void *p) { return (DG_GL const unsigned char *)(unsigned long long)p; }
__device__ __forceinline__ const GVecD *mvx_level0(const unsigned char *blob, int nLvCount) {
    const unsigned char *p = blob + 8;
    for (int i = nLvCount - 1; i >= 1; i--) p += *(const int *)p;
    return (const GVecD *)(p + 4);
}

struct PlaneG { // one plane of the clip / of level 0 of the super frame
    int W, H, WB, HB;        // frame dims, block-covered dims
    int blkW, blkH, ovX, ovY, stepX, stepY;
    int hpadPel, vpadPel;    // super padding * pel, in sub-pel units
    int subX, subY;          // log2 subsampling of this plane relative to luma
    long long srcPitch, supPitch, dstPitch, supPlaneStride; // bytes
    int thIdx;               // 0 luma threshold, 1 chroma threshold
    int process;
    int limit;
    long long shadow;        // 16-bit luma: byte distance to the copy of the super plane shifted left by one sample (mvx_degrain_set_ref_shadow), 0 = none
};

// MVFrame.cpp:1686-1704,1732-1734 mvpGetPointer as a byte offset inside the super plane (level 0)
__device__ __forceinline__ unsigned sup_offset(const PlaneG &g, int pel, int logPel, int bps, int nX, int nY) {
    nX += g.hpadPel; nY += g.vpadPel;
    const int m = pel - 1;
    const int idx = (nX & m) | ((nY & m) << logPel);
    return (unsigned)(idx * g.supPlaneStride + (long long)(nY >> logPel) * g.supPitch + (long long)(nX >> logPel) * bps);
}

// Pointers that come out of job tables are generic ("flat") to the compiler; the wide helpers take global-address-space pointers.
__device__ __forceinline__ DG_GL unsigned char *dg_glw(void *p) { return (DG_GL unsigned char *)(unsigned long long)p; }
typedef unsigned dg_uv4 __attribute__((ext_vector_type(4), aligned(1)));
typedef unsigned dg_uv2 __attribute__((ext_vector_type(2), aligned(1)));
typedef unsigned dg_uv1 __attribute__((aligned(1)));
typedef unsigned short dg_uh1 __attribute__((aligned(1)));

// ---- W samples of type T (1, 2, 4, 8, 16 or 32 bytes) at an arbitrarily aligned address: the one family of wide sample loads and stores.
// The bytes as dwords first and the samples out of them later, so that several loads can be in flight before the first one is unpacked
template <typename T, int W> struct DgRaw { unsigned d[(W * (int)sizeof(T) + 3) / 4]; };
template <typename T, int W> __device__ __forceinline__ DgRaw<T, W> dg_load_raw(DG_GL const unsigned char *p) {
    constexpr int BYTES = W * (int)sizeof(T);
    static_assert(BYTES == 1 || BYTES == 2 || BYTES == 4 || BYTES == 8 || BYTES == 16 || BYTES == 32, "1, 2, 4, 8, 16 or 32 bytes");
    DgRaw<T, W> r;
    if constexpr (BYTES >= 16) {
#pragma unroll
        for (int k = 0; k < BYTES / 16; k++) { dg_uv4 t = *(DG_GL const dg_uv4 *)(p + 16 * k); r.d[4 * k] = t[0]; r.d[4 * k + 1] = t[1]; r.d[4 * k + 2] = t[2]; r.d[4 * k + 3] = t[3]; }
    } else if constexpr (BYTES == 8) { dg_uv2 t = *(DG_GL const dg_uv2 *)p; r.d[0] = t[0]; r.d[1] = t[1]; }
    else if constexpr (BYTES == 4) r.d[0] = *(DG_GL const dg_uv1 *)p;
    else if constexpr (BYTES == 2) r.d[0] = *(DG_GL const dg_uh1 *)p;
    else r.d[0] = *p;
    return r;
}
template <typename T, int W> __device__ __forceinline__ int dg_sample(const DgRaw<T, W> &r, int i) {
    return sizeof(T) == 2 ? (int)((r.d[i >> 1] >> (16 * (i & 1))) & 0xffffu) : (int)((r.d[i >> 2] >> (8 * (i & 3))) & 0xffu);
}
// both steps at once: the samples widened to int
template <typename T, int W> __device__ __forceinline__ void dg_load(DG_GL const unsigned char *p, int *o) {
    const DgRaw<T, W> r = dg_load_raw<T, W>(p);
#pragma unroll
    for (int i = 0; i < W; i++) o[i] = dg_sample(r, i);
}
// N consecutive ints (dword-aligned address)
typedef int dg_iv4 __attribute__((ext_vector_type(4), aligned(4)));
typedef int dg_iv2 __attribute__((ext_vector_type(2), aligned(4)));
template <int N> __device__ __forceinline__ void dg_load_ints(DG_GL const unsigned char *p, int *o) {
    if (N >= 4) {
#pragma unroll
        for (int k = 0; k < N / 4; k++) { const dg_iv4 t = *(DG_GL const dg_iv4 *)(p + 16 * k); o[4 * k] = t[0]; o[4 * k + 1] = t[1]; o[4 * k + 2] = t[2]; o[4 * k + 3] = t[3]; }
    } else if (N == 2) { const dg_iv2 t = *(DG_GL const dg_iv2 *)p; o[0] = t[0]; o[1] = t[1]; }
    else o[0] = *(DG_GL const int *)p;
}
// W ints packed to samples of type T and stored
template <typename T, int W> __device__ __forceinline__ void dg_store(DG_GL unsigned char *p, const int *v) {
    constexpr int BYTES = W * (int)sizeof(T);
    DgRaw<T, W> r;
#pragma unroll
    for (int k = 0; k < (BYTES + 3) / 4; k++) r.d[k] = 0;
#pragma unroll
    for (int i = 0; i < W; i++) {
        if (sizeof(T) == 2) r.d[i >> 1] |= (unsigned)v[i] << (16 * (i & 1));
        else r.d[i >> 2] |= (unsigned)v[i] << (8 * (i & 3));
    }
    if constexpr (BYTES >= 16) {
#pragma unroll
        for (int k = 0; k < BYTES / 16; k++) { dg_uv4 t = { r.d[4 * k], r.d[4 * k + 1], r.d[4 * k + 2], r.d[4 * k + 3] }; *(DG_GL dg_uv4 *)(p + 16 * k) = t; }
    } else if constexpr (BYTES == 8) { dg_uv2 t = { r.d[0], r.d[1] }; *(DG_GL dg_uv2 *)p = t; }
    else if constexpr (BYTES == 4) *(DG_GL dg_uv1 *)p = r.d[0];
    else if constexpr (BYTES == 2) *(DG_GL dg_uh1 *)p = (unsigned short)r.d[0];
    else *p = (unsigned char)r.d[0];
}

// SimpleResize.cpp:62-121, uint8_t form, at one output sample whose table values are at hand: rows r0 / r1 (byte offsets), column o,
// vertical weights wt / wb, horizontal weights wl / wr.  PTR: a generic or a global-address-space byte pointer.
template <typename PTR> __device__ __forceinline__ int fps_upsize_u8(PTR m, int r0, int r1, int o, int wt, int wb, int wl, int wr) {
    const int a = (unsigned char)((m[r0 + o] * wt + m[r1 + o] * wb + 8192) >> 14), b = (unsigned char)((m[r0 + o + 1] * wt + m[r1 + o + 1] * wb + 8192) >> 14);
    return (unsigned char)((a * wl + b * wr + 8192) >> 14);
}

// Fakery.c:52-58,103-107,144-146 fgopIsUsable, the count part: this thread's share (stride 256) of the n level-0 blocks from `first` on whose SAD
// exceeds thscd1.  Global-address-space loads, four in flight, so that a wave does not wait for each 16-byte record on its own.
__device__ __forceinline__ int fps_count_over(const unsigned char *blob, int nLvCount, int first, int n, long long thscd1) {
    DG_GL const unsigned char *v = dg_gl(mvx_level0(blob, nLvCount)) + 16 * (long long)first + 8;
    int c = 0, i = threadIdx.x;
    for (; i + 768 < n; i += 1024) {
        const long long s0 = *(DG_GL const long long *)(v + 16 * i), s1 = *(DG_GL const long long *)(v + 16 * (i + 256));
        const long long s2 = *(DG_GL const long long *)(v + 16 * (i + 512)), s3 = *(DG_GL const long long *)(v + 16 * (i + 768));
        c += (s0 > thscd1) + (s1 > thscd1) + (s2 > thscd1) + (s3 > thscd1);
    }
    for (; i < n; i += 256) c += *(DG_GL const long long *)(v + 16 * i) > thscd1 ? 1 : 0;
    return c;
}
// fgopIsUsable of N vector fields by one workgroup of 256 threads, all of which call: every field has validity == 1 && !(count(sad > thscd1) >
// thscd2).  `want` (uniform) false: not usable, and no blob is dereferenced.  The decision is returned to thread 0 only (false elsewhere).
template <int N> __device__ __forceinline__ bool fps_block_usable(const unsigned char *const (&blob)[N], bool want, int nLvCount, int nBlk, long long thscd1, int thscd2) {
    __shared__ int cnt[N];
    if (threadIdx.x < N) cnt[threadIdx.x] = 0;
    __syncthreads();
    if (want) for (int d = 0; d < N; d++) atomicAdd(&cnt[d], fps_count_over(blob[d], nLvCount, 0, nBlk, thscd1));
    __syncthreads();
    bool ok = threadIdx.x == 0 && want;
    for (int d = 0; d < N; d++) ok = ok && ((const int *)blob[d])[1] == 1 && !(cnt[d] > thscd2);
    return ok;
}
__device__ __forceinline__ bool fps_block_usable(const unsigned char *blob, bool want, int nLvCount, int nBlk, long long thscd1, int thscd2) {
    const unsigned char *const one[1] = { blob };
    return fps_block_usable(one, want, nLvCount, nBlk, thscd1, thscd2);
}

// MaskFun.cpp:85-90 ByteOccMask, the value that is maxed into the mask.  fGamma 1 has no pow (the interpolating filters, which pass the
// constant, keep exactly their expression); otherwise the device's double pow, and a product beyond the int range -- where the reference's
// cast is undefined -- saturates to 255 (mv.Mask's divergence 3, mvtools_amd.h)
__device__ __forceinline__ int fps_occlusion_value(int o, double norm, double gamma) {
    if (gamma == 1.0) return min((int)(255 * o * norm), 255);
    const double l = 255 * pow(o * norm, gamma);
    return l >= 255.0 ? 255 : (int)l;
}
// MaskFun.cpp:86-130 MakeVectorOcclusionMaskTime for block (bx, by) = i: the occlusion against its right and bottom
// neighbours, scatter-maxed into the int plane m (pitch XP; zeroed before).  dir 1 = isBackward; time256 is the mask's own time
// (256 - t for the backward mask); ml is dMaskNormDivider.  Only maxima are taken, so the order of the reference's loops does not matter.
__device__ __forceinline__ void fps_occlusion_block(const GVecD *vec, int i, int bx, int by, int nBlkX, int nBlkY, int dir, int time256, int stepX, int stepY,
                                                    int nPel, double ml, int *m, int XP, double gamma = 1.0) {
    const int tX = time256 * 16 / (stepX * nPel), tY = time256 * 16 / (stepY * nPel);
    const double nX = 80.0 / (ml * stepX * nPel), nY = 80.0 / (ml * stepY * nPel);
    const int vx = vec[i].x, vy = vec[i].y;
    if (bx < nBlkX - 1) {
        const int vx1 = vec[i + 1].x;
        if (vx1 < vx) {
            const int o = vx - vx1;
            const int minb = dir ? max(0, bx + 1 - o * tX / 4096) : bx;
            const int maxb = dir ? bx + 1 : min(bx + 1 - o * tX / 4096, nBlkX - 1);
            const int val = fps_occlusion_value(o, nX, gamma);
            for (int b = minb; b <= maxb; b++) atomicMax(&m[b + by * XP], val);
        }
    }
    if (by < nBlkY - 1) {
        const int vy1 = vec[i + nBlkX].y;
        if (vy1 < vy) {
            const int o = vy - vy1;
            const int minb = dir ? max(0, by + 1 - o * tY / 4096) : by;
            const int maxb = dir ? by + 1 : min(by + 1 - o * tY / 4096, nBlkY - 1);
            const int val = fps_occlusion_value(o, nY, gamma);
            for (int b = minb; b <= maxb; b++) atomicMax(&m[bx + b * XP], val);
        }
    }
}
// MaskFun.cpp:38-80 CheckAndPadSmallY / CheckAndPadMaskSmall: the small-field cell that padded cell (x, y) clones -- the right clone
// first, then the bottom clone of the padded row
__device__ __forceinline__ int fps_pad_source(int x, int y, int nBlkX, int nBlkY, int XP) { return min(x, nBlkX - 1) + min(y, nBlkY - 1) * XP; }

// SimpleResize.cpp:27-57 InitTables (same float arithmetic)
static void bf_tables(int *offsets, int *weights, int out, int in) {
    const float leftmost = 0.5f, rightmost = in - 0.5f;
    const int leftmost_idx = std::max((int)leftmost, 0), rightmost_idx = std::min((int)rightmost, in - 1);
    for (int i = 0; i < out; i++) {
        const float position = (i + 0.5f) * (float)in / (float)out;
        float weight; int offset;
        if (position <= leftmost) { offset = leftmost_idx; weight = 0.0f; }
        else if (position >= rightmost) { offset = rightmost_idx - 1; weight = 1.0f; }
        else { offset = (int)(position - leftmost); weight = position - leftmost - offset; }
        offsets[i] = offset;
        weights[i] = (int)(weight * 16384);
    }
}
static long long bf_gcd(long long x, long long y) { while (y) { long long t = x % y; x = y; y = t; } return x; }

// ------------------------------------------------------------------------------------------------ host helpers

// the scene-change thresholds of a filter from its arguments: MV_DEFAULT_SCD1 / MV_DEFAULT_SCD2, then MVAnalysisData.c:7-31 scaleThSCD with
// its limit check.  unscaled: thscd1 before the scaling (Degrain and Compensate scale thsad by the same ratio)
static int mvx_resolve_thscd(const char *name, int64_t arg1, int32_t arg2, const mvx_analysis_data *ad, int64_t *thscd1, int32_t *thscd2, char *err,
                             int64_t *unscaled = nullptr) {
    const int maxSAD = 8 * 8 * 255;
    *thscd1 = arg1 == MVX_UNSET ? 400 : arg1;
    *thscd2 = arg2 == MVX_UNSET ? 130 : arg2;
    if (*thscd1 > maxSAD) MVX_FAIL("%s: thscd1 can be at most %d.", name, maxSAD);
    if (unscaled) *unscaled = *thscd1;
    mvx_scale_thscd(thscd1, thscd2, ad);
    return MVX_OK;
}

// the checks on mvbw / mvfw that every two-clip filter makes after comparing their geometry (MVBlockFPS.c:844-871, MVFlowInter.c:571-598,
// MVFlowBlur.c:440-467; FlowFPS lacks the first in the reference and then reads negative frame numbers: rejected here on purpose)
static int mvx_pair_checks(const char *name, const mvx_analysis_data *bw, const mvx_analysis_data *fw, char *err) {
    if (bw->nDeltaFrame <= 0 || fw->nDeltaFrame <= 0) MVX_FAIL("%s: cannot use motion vectors with absolute frame references.", name);
    if (bw->nDeltaFrame != fw->nDeltaFrame) MVX_FAIL("%s: mvbw and mvfw must be generated with the same delta.", name);
    if (!bw->isBackward) MVX_FAIL("%s: mvbw must be generated with isb=True.", name);
    if (fw->isBackward) MVX_FAIL("%s: mvfw must be generated with isb=False.", name);
    return MVX_OK;
}

// "wrong source or super clip frame size": the vectors against the super clip, and with `width` also against the clip's own width
static bool mvx_super_fits(const mvx_analysis_data *ad, const mvx_super_info &si, bool width) {
    return ad->nHeight == si.height && ad->nWidth == si.super_width - si.hpad * 2 && (!width || ad->nWidth == si.width) && ad->nPel == si.pel;
}

// frame-rate conversion of BlockFPS and FlowFPS (MVBlockFPS.c:703-718,888-909, MVFlowFPS.c:547-561,714-744): fa / fb = input rate / output
// rate in lowest terms, the output clip's rate and frame count.  num / den as passed: MVX_UNSET -> 25 / 1, 0 -> double the input rate
struct FpsRate { long long fa, fb, outNum, outDen; int outFrames; };
static void fps_rate_init(FpsRate &r, long long num, long long den, long long fps_num, long long fps_den, int num_frames) {
    if (num == MVX_UNSET) num = 25;
    if (den == MVX_UNSET) den = 1;
    if (num == 0 || den == 0) { num = fps_num * 2; den = fps_den; }
    r.fa = den * fps_num; r.fb = num * fps_den;
    const long long g = bf_gcd(r.fa, r.fb);
    r.fa /= g; r.fb /= g;
    if (num <= 0 || den <= 0) { r.outNum = 0; r.outDen = 1; } // setFPS
    else { const long long x = bf_gcd(num, den); r.outNum = num / x; r.outDen = den / x; }
    r.outFrames = (int)(1 + (num_frames - 1) * r.fb / r.fa);
}
// output frame n -> the input frames it lies between and its time position (MVBlockFPS.c:245-254,278-292, MVFlowFPS.c:92-99,125-134)
static void fps_rate_map(const FpsRate &r, int delta, int n, int *nleft, int *nright, int *time256) {
    *nleft = (int)(n * r.fa / r.fb);
    int t = (int)(((double)n * r.fa / r.fb - *nleft) * 256 + 0.5);
    if (delta > 1) t = t / delta;
    *nright = *nleft + delta;
    *time256 = t;
}

// the small fields padded until they cover the frame, and the size the upsizer stretches them to, luma / chroma (MVBlockFPS.c:936-949,
// MVFlowInter.c:651-665, MVFlowFPS.c:804-816, MVFlow.cpp:535-546)
static void fps_padded_grid(const mvx_analysis_data *ad, int *XP, int *YP, int nWidthP[2], int nHeightP[2]) {
    const int stepX = ad->nBlkSizeX - ad->nOverlapX, stepY = ad->nBlkSizeY - ad->nOverlapY;
    *XP = ad->nBlkX; *YP = ad->nBlkY;
    while (*XP * stepX + ad->nOverlapX < ad->nWidth) (*XP)++;
    while (*YP * stepY + ad->nOverlapY < ad->nHeight) (*YP)++;
    nWidthP[0] = *XP * stepX + ad->nOverlapX; nHeightP[0] = *YP * stepY + ad->nOverlapY;
    nWidthP[1] = nWidthP[0] / ad->xRatioUV; nHeightP[1] = nHeightP[0] / ad->yRatioUV;
}
// a parameter block on the device
template <typename PARAMS> static int fps_upload_params(DevBuf<PARAMS> &d, const PARAMS &P) {
    HIP_CHECK(d.reserve(1));
    const hipError_t e = hipMemcpy(d.p, &P, sizeof(PARAMS), hipMemcpyHostToDevice);
    if (e != hipSuccess) d.release(); // (handles take an existing block for an uploaded one)
    HIP_CHECK(e);
    return MVX_OK;
}
// the upsizer tables from the P.XP x P.YP small fields to nWidthP / nHeightP (luma, chroma) on the device, then P, which points into them
template <typename PARAMS> static int fps_upload_tables(DevBuf<int> &tables, DevBuf<PARAMS> &d, PARAMS &P, const int nWidthP[2], const int nHeightP[2]) {
    const int n = nWidthP[0] + nWidthP[1] + nHeightP[0] + nHeightP[1];
    std::vector<int> t(2 * n);
    int *o = t.data(), *w = t.data() + n, pos = 0;
    HIP_CHECK(tables.reserve(2 * (size_t)n));
    for (int c = 0; c < 2; c++) {
        bf_tables(o + pos, w + pos, nWidthP[c], P.XP); P.hOff[c] = tables.p + pos; P.hW[c] = tables.p + n + pos; pos += nWidthP[c];
        bf_tables(o + pos, w + pos, nHeightP[c], P.YP); P.vOff[c] = tables.p + pos; P.vW[c] = tables.p + n + pos; pos += nHeightP[c];
    }
    HIP_CHECK(hipMemcpy(tables.p, t.data(), sizeof(int) * 2 * n, hipMemcpyHostToDevice));
    return fps_upload_params(d, P);
}

// the three planes of the clip and of level 0 of its super clip; a clip with fewer planes repeats plane 0's pitches
static void fps_fill_planes(PlaneG pl[3], const mvx_analysis_data *ad, const mvx_super_info &si, const ptrdiff_t src_pitch[3], const ptrdiff_t super_pitch[3],
                            const ptrdiff_t dst_pitch[3]) {
    const int xSub = mvx_ilog2(si.xRatioUV), ySub = mvx_ilog2(si.yRatioUV);
    for (int p = 0; p < 3; p++) {
        PlaneG &g = pl[p];
        const int sx = p ? xSub : 0, sy = p ? ySub : 0, q = p < si.num_planes ? p : 0;
        g.subX = sx; g.subY = sy;
        g.W = ad->nWidth >> sx; g.H = ad->nHeight >> sy;
        g.blkW = ad->nBlkSizeX >> sx; g.blkH = ad->nBlkSizeY >> sy;
        g.ovX = ad->nOverlapX >> sx; g.ovY = ad->nOverlapY >> sy;
        g.stepX = g.blkW - g.ovX; g.stepY = g.blkH - g.ovY;
        g.WB = (ad->nBlkX * (ad->nBlkSizeX - ad->nOverlapX) + ad->nOverlapX) >> sx;
        g.HB = (ad->nBlkY * (ad->nBlkSizeY - ad->nOverlapY) + ad->nOverlapY) >> sy;
        g.hpadPel = (si.hpad >> sx) * si.pel; g.vpadPel = (si.vpad >> sy) * si.pel; // MVFrame.cpp:1334-1335,1775-1779; the Finest frame's nOffsetY / nOffsetUV (MVFlowInter.c:218-219)
        g.srcPitch = src_pitch ? src_pitch[q] : 0;
        g.supPitch = super_pitch[q];
        g.dstPitch = dst_pitch[q];
        g.supPlaneStride = g.supPitch * (long long)((si.height >> sy) + 2 * (si.vpad >> sy));
        g.thIdx = p ? 1 : 0;
        g.process = 1; g.limit = si.bits > 16 ? 255 : (1 << si.bits) - 1; // (a float clip's limits are on the 8-bit scale)
        g.shadow = 0;
    }
}

// ---- the layout contract of the vector consumers (include/mvtools_amd.h, "Plane layouts").  Clip-side planes -- the clip planes a filter
// reads and the planes it writes: a pitch holds a row of its plane and is a multiple of the sample size, and so is every plane address; U and
// V may differ.  Super planes: what mvx_super_frames writes -- pitches that hold a row and are multiples of 16 bytes, U and V alike, planes on
// 16-byte boundaries.  *_create checks the pitches, *_frames the addresses, before anything is uploaded or launched.
// the pitches of the planes `what` ("src", "clip", "dst") of pl[0..nplanes), sample size bps
static int fps_check_pitches(const char *what, const PlaneG pl[3], int nplanes, const ptrdiff_t pitch[3], int bps, char *err) {
    for (int p = 0; p < nplanes; p++) {
        const long long row = (long long)pl[p].W * bps;
        if (pitch[p] < row || pitch[p] % bps) MVX_FAIL("%s pitch of plane %d must hold a row of %lld bytes and be a multiple of the sample size.", what, p, row);
    }
    return MVX_OK;
}
// the pitches of the super planes
static int fps_check_super_pitches(const mvx_super_info &si, const ptrdiff_t super_pitch[3], char *err) {
    const int bps = (si.bits + 7) / 8;
    for (int p = 0; p < si.num_planes; p++) {
        const long long row = (long long)si.plane_width[p] * bps;
        if (super_pitch[p] < row || super_pitch[p] % 16) MVX_FAIL("super pitch of plane %d must hold a row of %lld bytes and be a multiple of 16 bytes.", p, row);
    }
    return MVX_OK;
}
// the addresses of one job's planes `what`: each a multiple of `align` bytes, and all there when `required` (planes a job may leave out --
// a reference outside the clip, the chroma of a super clip without chroma -- are NULL and pass)
static int fps_check_planes(const char *fn, const char *what, const void *const *planes, int nplanes, int align, bool required) {
    for (int p = 0; p < nplanes; p++) {
        if (!planes[p] && required) { mvx_set_error("%s: %s plane %d is required", fn, what, p); return MVX_E_ARG; }
        if ((uintptr_t)planes[p] % (uintptr_t)align) { mvx_set_error("%s: %s plane %d must be aligned to %d bytes", fn, what, p, align); return MVX_E_ARG; }
    }
    return MVX_OK;
}

// ---- launches of the kernels that produce CW consecutive samples per thread, 64 x 4 threads per workgroup
// the widest segment of at most 16 bytes that divides a plane of W samples
static int fps_segment(int bps, int W) { int cw = 16 / bps; while (cw > 1 && W % cw) cw >>= 1; return cw; }
// one launch for the luma planes of all jobs and one for both chroma planes of all jobs (the two classes differ in the segment and in the
// upsizer tables): launch(grid, cw, first plane, planes per job) with cw = cwOf(first plane)
template <typename CWOF, typename F> static void fps_classes(const PlaneG pl[3], int nplanes, int nframes, CWOF &&cwOf, F &&launch) {
    for (int cls = 0; cls < (nplanes > 1 ? 2 : 1); cls++) {
        const int p0 = cls, npl = cls ? 2 : 1, cw = cwOf(p0);
        launch(dim3((unsigned)((pl[p0].W / cw + 63) / 64), (unsigned)((pl[p0].H + 3) / 4), (unsigned)(nframes * npl)), cw, p0, npl);
    }
}
// (bytes per sample, segment) -> f(fps_type<T>(), std::integral_constant<int, CW>()) for the segments MINW .. 16 bytes of uint8_t / uint16_t; a
// generic lambda launches kernel<typename decltype(t)::type, decltype(w)::value>.  Only these combinations are instantiated.
template <typename T> struct fps_type { typedef T type; };
template <int MINW, typename T, int W, typename F> static void fps_dispatch_width(int cw, F &f) {
    if constexpr (W > MINW) { if (cw < W) return fps_dispatch_width<MINW, T, W / 2>(cw, f); }
    f(fps_type<T>(), std::integral_constant<int, W>());
}
template <int MINW, typename F> static void fps_dispatch(int bps, int cw, F &&f) {
    if (bps == 1) fps_dispatch_width<MINW, uint8_t, 16>(cw, f); else fps_dispatch_width<MINW, uint16_t, 8>(cw, f);
}
// the segments MINW .. 4 of float32 samples (16 bytes at most, like the others).  On its own, so that a kernel gets a float form only where
// its caller asks for one
template <int MINW, typename F> static void fps_dispatch_float(int cw, F &&f) { fps_dispatch_width<MINW, float, 4>(cw, f); }
