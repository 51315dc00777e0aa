// mvx_flow.hip -- mv.FlowInter and mv.FlowFPS on gfx950; mv.Flow and mv.FlowBlur on the same machinery (second half of the file).
//
// The reference builds, per output frame and plane class, full-resolution int16 vector planes (SimpleResize.cpp:60-121 on the
// block-resolution fields of MaskFun.cpp:169-203) and full-resolution occlusion masks, then runs FlowInterSimple / FlowInter /
// FlowInterExtra (MaskFun.cpp:374-555) over them against the Finest frame (MVFlowInter.c:80-452, MVFlowFPS.c:86-524,
// MVFlowFPSHelper.c:49-93).  Here none of the full-resolution planes exists: per job, tiny kernels decide usability and compute the
// padded small fields; ONE gather pass then upsizes the vectors and masks at each output sample with the reference's integer tables
// and rounding, and fetches the compensated samples straight from the super frames (sup_offset interleaves the pel^2 sub-planes
// exactly as mv.Finest does), so the Finest frame is never built either:
//   flow_usable_kernel : per (job, blob) -> usable flags; fl_state turns a job's four flags into its formula (Simple / regular / Extra)
//                        or the Blend / copy fallback
//   flow_occ_kernel    : per (job, direction, block) -> occlusion scatter-max (BlockFPS's code, mvx_fps_shared.h)
//   flow_cells_kernel  : per (job, padded cell) -> padded vector cells (CheckAndPadSmallY) and padded mask bytes (CheckAndPadMaskSmall)
//   flow_kernel        : per CW consecutive output samples -> the interpolated samples, one wide store; one launch for the luma planes
//                        of all jobs and one for both chroma planes of all jobs (the two classes differ in CW and in the upsizer tables)
#include "mvx_fps_shared.h"
#include "mvx_flow_float_rule.h"

enum { FL_SIMPLE = 0, FL_REGULAR = 1, FL_EXTRA = 2, FL_FALLBACK = -1 };

struct FLParams {
    int nplanes, pel, logPel, bits, bps;
    int nBlkX, nBlkY, nBlk, nLvCount, stepX, stepY;
    int XP, YP;                           // padded small-field grid (nBlkXP, nBlkYP)
    int isFPS, maskmode, blend;
    int halfX, halfY;                     // VectorSmallMaskYToHalfUV: chroma vector = luma >> 1 along an axis with ratio 2
    long long thscd1; int thscd2;
    double ml;
    int limW[2], limH[2];                 // the int16 resizer's limit_width / limit_height: luma / chroma frame size
    PlaneG pl[3];
    const int *hOff[2], *hW[2], *vOff[2], *vW[2]; // SimpleResize tables, luma / chroma upsizer
    long long clipPitch[3];
};
struct FLJob {
    const unsigned char *supL[3], *supR[3];  // super frames nleft / nright (the reference's pSrc / pRef Finest frames)
    const unsigned char *blobF, *blobB;      // mvfw at nright, mvbw at nleft
    const unsigned char *blobFF, *blobBB;    // mvfw at nleft, mvbw at nright (Extra)
    const unsigned char *clipL[3], *clipR[3];
    unsigned char *dst[3];
    int time256, copy;                       // copy: 1 / 2 = the clip frame left / right (FlowFPS at time256 0 / 256, MVFlowFPS.c:138-142)
};
// one padded small-field cell: the B, F, BB, FF vectors as int16 (MakeVectorSmallMasks stores them into int16_t planes), x in the low half
struct FLCell { short bx, by, fx, fy, bbx, bby, ffx, ffy; };
static_assert(sizeof(FLCell) == 16, "cell layout");
__device__ __forceinline__ int fl_lo(int w) { return (int)(short)(w & 0xffff); }
__device__ __forceinline__ int fl_hi(int w) { return w >> 16; }

// the wide helpers move at least two bytes: a single 8-bit sample goes on its own.  T = float (Flow and FlowBlur on float clips, second half
// of the file): the int holds the sample's 32 bits as they are -- no float operation sees a sample that is only moved, so NaN payloads and
// signed zeros survive -- and W of them are one store of 4, 8 or 16 bytes
template <typename T, int W> __device__ __forceinline__ void fl_load(DG_GL const unsigned char *p, int *o) {
    if constexpr (sizeof(T) == 4) {
        const DgRaw<T, W> r = dg_load_raw<T, W>(p);
#pragma unroll
        for (int i = 0; i < W; i++) o[i] = (int)r.d[i];
    } else if constexpr (W * sizeof(T) == 1) o[0] = *p; else dg_load<T, W>(p, o);
}
template <typename T, int W> __device__ __forceinline__ void fl_store(DG_GL unsigned char *p, const int *v) {
    if constexpr (sizeof(T) == 4) {
        static_assert(W == 1 || W == 2 || W == 4, "4, 8 or 16 bytes");
        if constexpr (W == 4) { const dg_uv4 t = { (unsigned)v[0], (unsigned)v[1], (unsigned)v[2], (unsigned)v[3] }; *(DG_GL dg_uv4 *)p = t; }
        else if constexpr (W == 2) { const dg_uv2 t = { (unsigned)v[0], (unsigned)v[1] }; *(DG_GL dg_uv2 *)p = t; }
        else *(DG_GL dg_uv1 *)p = (unsigned)v[0];
    } else if constexpr (W * sizeof(T) == 1) *p = (unsigned char)v[0]; else dg_store<T, W>(p, v);
}

// per (job, blob): Fakery.c:52-58,103-107,144-146 fgopIsUsable of mvfw at nright, mvbw at nleft, mvfw at nleft, mvbw at nright -> flags[job][4];
// 0 for a blob the job does not read (copies, frames outside the clip, the extra blobs of FlowFPS mask 0 / 1)
__global__ __launch_bounds__(256) void flow_usable_kernel(const FLParams *Pp, const FLJob *jobs, int *flags) {
    const FLParams &P = *Pp;
    const int f = blockIdx.x, k = blockIdx.y;
    const FLJob &J = jobs[f];
    const unsigned char *blob = k == 0 ? J.blobF : k == 1 ? J.blobB : k == 2 ? J.blobFF : J.blobBB;
    const bool want = !J.copy && J.supL[0] && J.supR[0] && blob && (k < 2 || !P.isFPS || P.maskmode == 2);
    const bool ok = fps_block_usable(blob, want, P.nLvCount, P.nBlk, P.thscd1, P.thscd2);
    if (threadIdx.x == 0) flags[f * 4 + k] = ok;
}
// the job's formula (MVFlowInter.c:109-138,245-276 / MVFlowFPS.c:153-166,314-354,385-435): the masks and B / F come from the main vectors, the
// extra blobs only pick the formula; FlowFPS mask 2 without usable extra vectors falls through to Simple (MVFlowFPS.c:435)
__device__ __forceinline__ int fl_state(const FLParams &P, const int *fl) {
    if (!fl[0] || !fl[1]) return FL_FALLBACK;
    const bool extra = fl[2] && fl[3];
    if (!P.isFPS) return extra ? FL_EXTRA : FL_REGULAR;
    if (P.maskmode == 1) return FL_REGULAR;
    return extra ? FL_EXTRA : FL_SIMPLE;
}

// MakeVectorOcclusionMaskTime for the B mask (isBackward, 256 - t) and the F mask (t) into int planes [job][F,B][YP*XP], zeroed before
__global__ __launch_bounds__(256) void flow_occ_kernel(const FLParams *Pp, const FLJob *jobs, const int *flags, int *small) {
    const FLParams &P = *Pp;
    const int f = blockIdx.z, dir = blockIdx.y; // dir 0 = forward mask, 1 = backward mask
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (fl_state(P, flags + 4 * f) < 0 || i >= P.nBlk) return;
    const FLJob &J = jobs[f];
    const GVecD *vec = mvx_level0(dir ? J.blobB : J.blobF, P.nLvCount);
    const int by = i / P.nBlkX, bx = i - by * P.nBlkX;
    fps_occlusion_block(vec, i, bx, by, P.nBlkX, P.nBlkY, dir, dir ? 256 - J.time256 : J.time256, P.stepX, P.stepY, P.pel, P.ml,
                        small + ((size_t)f * 2 + dir) * P.XP * P.YP, P.XP);
}

// MaskFun.cpp:38-60 CheckAndPadSmallY: cells right of the field take min(vx, 0) and the row's vy, cells below take the (padded) row's vx and min(vy, 0)
__device__ __forceinline__ void fl_padded(const GVecD *v, int s, bool right, bool below, short &vx, short &vy) {
    vx = (short)v[s].x; vy = (short)v[s].y;
    if (right) vx = min(vx, (short)0);
    if (below) vy = min(vy, (short)0);
}
__global__ __launch_bounds__(256) void flow_cells_kernel(const FLParams *Pp, const FLJob *jobs, const int *flags, const int *small, FLCell *cells, unsigned char *masks) {
    const FLParams &P = *Pp;
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int st = fl_state(P, flags + 4 * f);
    const int cellsN = P.XP * P.YP;
    if (st < 0 || i >= cellsN) return;
    const FLJob &J = jobs[f];
    const int y = i / P.XP, x = i - y * P.XP;
    const int s = fps_pad_source(x, y, P.nBlkX, P.nBlkY, P.XP), sb = min(x, P.nBlkX - 1) + min(y, P.nBlkY - 1) * P.nBlkX;
    const bool right = x >= P.nBlkX, below = y >= P.nBlkY;
    FLCell c;
    fl_padded(mvx_level0(J.blobB, P.nLvCount), sb, right, below, c.bx, c.by);
    fl_padded(mvx_level0(J.blobF, P.nLvCount), sb, right, below, c.fx, c.fy);
    if (st == FL_EXTRA) {
        fl_padded(mvx_level0(J.blobBB, P.nLvCount), sb, right, below, c.bbx, c.bby);
        fl_padded(mvx_level0(J.blobFF, P.nLvCount), sb, right, below, c.ffx, c.ffy);
    } else {
        c.bbx = c.bby = c.ffx = c.ffy = 0;
    }
    cells[(size_t)f * cellsN + i] = c;
    const int *mF = small + ((size_t)f * 2 + 0) * cellsN, *mB = small + ((size_t)f * 2 + 1) * cellsN;
    unsigned char *o = masks + (size_t)f * 2 * cellsN;
    o[i] = (unsigned char)mF[s];
    o[cellsN + i] = (unsigned char)mB[s];
}

// SimpleResize.cpp:60-121 for int16 fields at one output sample: the vertical pass rounds per small-field column, then the horizontal
// pass rounds and clamps to [lo, hi]
__device__ __forceinline__ int fl_vup(int s1a, int s2a, int s1b, int s2b, int wt, int wb, int wl, int wr, int lo, int hi) {
    const int a = (short)((s1a * wt + s2a * wb + 8192) >> 14), b = (short)((s1b * wt + s2b * wb + 8192) >> 14);
    const int r = (a * wl + b * wr + 8192) >> 14;
    return (short)max(lo, min(r, hi));
}

template <typename T>
__device__ __forceinline__ int fl_fetch(const FLParams &P, const PlaneG &g, const unsigned char *sup, int X, int Y) {
    if constexpr (sizeof(T) == 4) return (int)*(DG_GL const unsigned *)dg_gl(sup + sup_offset(g, P.pel, P.logPel, 4, X, Y)); // the bits of a float sample
    else return *(DG_GL const T *)dg_gl(sup + sup_offset(g, P.pel, P.logPel, (int)sizeof(T), X, Y));
}

// one thread per CW consecutive samples of one row of plane class p0 .. p0 + npl - 1.  T = float (mvx_flowinter_create_float,
// mvx_flowfps_create_float; the rules are in include/mvtools_amd.h and mvx_flow_float_rule.h): the vectors, the masks and the fetch positions
// are the integer filter's, the fetched 32 bits go through the rule header as float32, a copy moves them untouched
template <typename T, int CW>
__global__ __launch_bounds__(256) void flow_kernel(const FLParams *Pp, const FLJob *jobs, const int *flags, const FLCell *cells, const unsigned char *masks,
                                                   int planeFirst, int planesPerFrame) {
    const FLParams &P = *Pp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * CW, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const FLJob &J = jobs[f];
    DG_GL unsigned char *dptr = dg_glw(J.dst[p] + (long long)y * g.dstPitch + (long long)x * (long long)sizeof(T));
    const int t = J.time256, st = fl_state(P, flags + 4 * f);
    int out[CW];
    if (st < 0) { // copy at FlowFPS's time256 0 / 256, else Blend or the left frame (MaskFun.cpp:349-371, MVFlowInter.c:403-446, MVFlowFPS.c:475-519)
        const long long co = (long long)y * P.clipPitch[p] + (long long)x * (long long)sizeof(T);
        int l[CW];
        if (J.copy == 2) { fl_load<T, CW>(dg_gl(J.clipR[p] + co), l); fl_store<T, CW>(dptr, l); return; }
        fl_load<T, CW>(dg_gl(J.clipL[p] + co), l);
        if (J.copy == 1 || !P.blend) { fl_store<T, CW>(dptr, l); return; }
        int r[CW];
        fl_load<T, CW>(dg_gl(J.clipR[p] + co), r);
#pragma unroll
        for (int i = 0; i < CW; i++) {
            if constexpr (sizeof(T) == 4) out[i] = __float_as_int(mvx_flf_blend(t, __int_as_float(l[i]), __int_as_float(r[i])));
            else out[i] = (int)(T)((l[i] * (256 - t) + r[i] * t) >> 8);
        }
        fl_store<T, CW>(dptr, out);
        return;
    }
    const int c = p ? 1 : 0;
    const int cellsN = P.XP * P.YP;
    const int wb = *(DG_GL const int *)dg_gl(P.vW[c] + y), wt = 16384 - wb;
    const int r0 = *(DG_GL const int *)dg_gl(P.vOff[c] + y) * P.XP, r1 = r0 + P.XP;
    int hO[CW], hWr[CW];
    dg_load_ints<CW>(dg_gl(P.hOff[c] + x), hO);
    dg_load_ints<CW>(dg_gl(P.hW[c] + x), hWr);
    DG_GL const unsigned char *cl = dg_gl(cells + (size_t)f * cellsN);
    DG_GL const unsigned char *mFp = dg_gl(masks + (size_t)f * 2 * cellsN), *mBp = mFp + cellsN;
    const int hx = c && P.halfX ? 1 : 0, hy = c && P.halfY ? 1 : 0;
    const int pel = P.pel, lp = P.logPel;
    const int yLo = -y * pel, yHi = (P.limH[c] - y) * pel - 1;
    const int Y = y << lp;
#pragma unroll
    for (int i = 0; i < CW; i++) {
        const int xi = x + i, o = hO[i], wr = hWr[i], wl = 16384 - wr;
        const int xLo = -xi * pel, xHi = (P.limW[c] - xi) * pel - 1;
        // the four cells around the sample: (row r0 / r1) x (column o / o + 1), B and F vectors as two dwords each
        const dg_iv2 a0 = *(DG_GL const dg_iv2 *)(cl + 16 * (r0 + o)), b0 = *(DG_GL const dg_iv2 *)(cl + 16 * (r0 + o + 1));
        const dg_iv2 a1 = *(DG_GL const dg_iv2 *)(cl + 16 * (r1 + o)), b1 = *(DG_GL const dg_iv2 *)(cl + 16 * (r1 + o + 1));
        const int vxB = fl_vup(fl_lo(a0[0]) >> hx, fl_lo(a1[0]) >> hx, fl_lo(b0[0]) >> hx, fl_lo(b1[0]) >> hx, wt, wb, wl, wr, xLo, xHi);
        const int vyB = fl_vup(fl_hi(a0[0]) >> hy, fl_hi(a1[0]) >> hy, fl_hi(b0[0]) >> hy, fl_hi(b1[0]) >> hy, wt, wb, wl, wr, yLo, yHi);
        const int vxF = fl_vup(fl_lo(a0[1]) >> hx, fl_lo(a1[1]) >> hx, fl_lo(b0[1]) >> hx, fl_lo(b1[1]) >> hx, wt, wb, wl, wr, xLo, xHi);
        const int vyF = fl_vup(fl_hi(a0[1]) >> hy, fl_hi(a1[1]) >> hy, fl_hi(b0[1]) >> hy, fl_hi(b1[1]) >> hy, wt, wb, wl, wr, yLo, yHi);
        const int mF = fps_upsize_u8(mFp, r0, r1, o, wt, wb, wl, wr), mB = fps_upsize_u8(mBp, r0, r1, o, wt, wb, wl, wr);
        const int X = xi << lp;
        const int dF = fl_fetch<T>(P, g, J.supL[p], X + ((vxF * t) >> 8), Y + ((vyF * t) >> 8));
        const int dB = fl_fetch<T>(P, g, J.supR[p], X + ((vxB * (256 - t)) >> 8), Y + ((vyB * (256 - t)) >> 8));
        int v;
        if (st == FL_SIMPLE) { // MaskFun.cpp:493-551 (time256 == 128 has its own formula; its vectors v >> 1 equal (v * 128) >> 8)
            if constexpr (sizeof(T) == 4) v = __float_as_int(mvx_flf_simple(t, __int_as_float(dF), __int_as_float(dB), mF, mB)); // one formula at every t
            else if (t == 128) v = (((dF + dB) << 8) + (dB - dF) * (mF - mB)) >> 9;
            else v = (((dF * (255 - mF) + dB * mF + 255) >> 8) * (256 - t) + ((dB * (255 - mB) + dF * mB + 255) >> 8) * t) >> 8;
        } else if (st == FL_REGULAR) { // MaskFun.cpp:374-414: the int64 products are non-negative and below 2^32
            const unsigned dF0 = (unsigned)fl_fetch<T>(P, g, J.supL[p], X, Y), dB0 = (unsigned)fl_fetch<T>(P, g, J.supR[p], X, Y);
            if constexpr (sizeof(T) == 4) {
                v = __float_as_int(mvx_flf_regular(t, __int_as_float(dF), __int_as_float(dB), __uint_as_float(dF0), __uint_as_float(dB0), mF, mB));
            } else {
                const unsigned uF = (unsigned)dF, uB = (unsigned)dB, kF = (unsigned)mF, kB = (unsigned)mB;
                const unsigned a = (uF * (255 - kF) + ((kF * (uB * (255 - kB) + kB * dF0) + 255) >> 8) + 255) >> 8;
                const unsigned b = (uB * (255 - kB) + ((kB * (uF * (255 - kF) + kF * dB0) + 255) >> 8) + 255) >> 8;
                v = (int)((a * (unsigned)(256 - t) + b * (unsigned)t) >> 8);
            }
        } else { // MaskFun.cpp:417-490
            const dg_iv2 c0 = *(DG_GL const dg_iv2 *)(cl + 16 * (r0 + o) + 8), d0 = *(DG_GL const dg_iv2 *)(cl + 16 * (r0 + o + 1) + 8);
            const dg_iv2 c1 = *(DG_GL const dg_iv2 *)(cl + 16 * (r1 + o) + 8), d1 = *(DG_GL const dg_iv2 *)(cl + 16 * (r1 + o + 1) + 8);
            const int vxBB = fl_vup(fl_lo(c0[0]) >> hx, fl_lo(c1[0]) >> hx, fl_lo(d0[0]) >> hx, fl_lo(d1[0]) >> hx, wt, wb, wl, wr, xLo, xHi);
            const int vyBB = fl_vup(fl_hi(c0[0]) >> hy, fl_hi(c1[0]) >> hy, fl_hi(d0[0]) >> hy, fl_hi(d1[0]) >> hy, wt, wb, wl, wr, yLo, yHi);
            const int vxFF = fl_vup(fl_lo(c0[1]) >> hx, fl_lo(c1[1]) >> hx, fl_lo(d0[1]) >> hx, fl_lo(d1[1]) >> hx, wt, wb, wl, wr, xLo, xHi);
            const int vyFF = fl_vup(fl_hi(c0[1]) >> hy, fl_hi(c1[1]) >> hy, fl_hi(d0[1]) >> hy, fl_hi(d1[1]) >> hy, wt, wb, wl, wr, yLo, yHi);
            const int dFF = fl_fetch<T>(P, g, J.supL[p], X + ((vxFF * t) >> 8), Y + ((vyFF * t) >> 8));
            const int dBB = fl_fetch<T>(P, g, J.supR[p], X + ((vxBB * (256 - t)) >> 8), Y + ((vyBB * (256 - t)) >> 8));
            if constexpr (sizeof(T) == 4) {
                v = __float_as_int(mvx_flf_extra(t, __int_as_float(dF), __int_as_float(dB), __int_as_float(dFF), __int_as_float(dBB), mF, mB));
            } else {
                const int mn = min(dB, dF), mx = max(dB, dF);
                const int medBB = max(mn, min(dBB, mx)), medFF = max(mn, min(dFF, mx));
                v = (((medBB * mF + dF * (255 - mF) + 255) >> 8) * (256 - t) + ((medFF * mB + dB * (255 - mB) + 255) >> 8) * t) >> 8;
            }
        }
        if constexpr (sizeof(T) == 4) out[i] = v; else out[i] = (int)(T)v; // float: v holds the result's 32 bits
    }
    fl_store<T, CW>(dptr, out);
}

// ------------------------------------------------------------------------------------------------ host object

struct mvx_flow {
    CallGuard guard;
    FLParams P;
    DevBuf<FLParams> dP;
    DevBuf<FLJob> dJobs;              // the per-job buffers hold exactly the largest call's jobs
    DevBuf<int> dFlags, dSmall, dTables;
    DevBuf<FLCell> dCells;
    DevBuf<unsigned char> dMasks;
    int nWidthP[2], nHeightP[2];
    int delta, time256;
    FpsRate rate;                     // FlowFPS; FlowInter: the clip's frame count and no rate
};

// MVAnalysisData.c:68-98 adataCheckSimilarity: every mismatching field overwrites the message, so the LAST one is reported
static bool flow_similarity(const mvx_analysis_data *a, const mvx_analysis_data *b, const char *name, char *err) {
    bool bad = false;
    auto msg = [&](const char *what) { snprintf(err, MVX_ERRLEN, "%s: mvbw and mvfw have different %s.", name, what); bad = true; };
    if (a->nWidth != b->nWidth) msg("widths");
    if (a->nHeight != b->nHeight) msg("heights");
    if (a->nBlkSizeX != b->nBlkSizeX || a->nBlkSizeY != b->nBlkSizeY) msg("block sizes");
    if (a->nPel != b->nPel) msg("pel precision");
    if (a->nOverlapX != b->nOverlapX || a->nOverlapY != b->nOverlapY) msg("overlap");
    if (a->xRatioUV != b->xRatioUV) msg("horizontal subsampling");
    if (a->yRatioUV != b->yRatioUV) msg("vertical subsampling");
    if (a->bitsPerSample != b->bitsPerSample) msg("bit depths");
    return bad;
}

// the two-clip checks FlowInter, FlowFPS and FlowBlur share after their own argument checks (MVFlowInter.c:540-574, MVFlowFPS.c:646-671,
// MVFlowBlur.c:410-470)
static int flow_pair_checks(const char *name, int64_t arg1, int32_t arg2, int64_t *thscd1, int32_t *thscd2, const mvx_analysis_data *bw,
                            const mvx_analysis_data *fw, char *err) {
    if (int rc = mvx_resolve_thscd(name, arg1, arg2, bw, thscd1, thscd2, err)) return rc;
    if (flow_similarity(bw, fw, name, err)) { mvx_set_error("%s", err); return MVX_E_ARG; }
    return mvx_pair_checks(name, bw, fw, err);
}

// the geometry of every flow filter: padded small fields and upsizer tables to nWidthP / nHeightP (MVFlowInter.c:651-678,
// MVFlowFPS.c:776-802, MVFlow.cpp:535-562), or with padded = false FlowBlur's unpadded fields and tables that end at the frame
// (MVFlowBlur.c:525-536), so that a frame the block grid does not cover gets a stretched grid
static int flow_geometry(FLParams &P, int nWidthP[2], int nHeightP[2], const char *name, int64_t thscd1, int32_t thscd2, const mvx_analysis_data *bw,
                         const mvx_super_info &si, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], bool padded,
                         char *err) {
    memset(&P, 0, sizeof(P));
    P.thscd1 = thscd1; P.thscd2 = thscd2;
    P.nplanes = (si.modeYUV & 6) && si.num_planes > 1 ? 3 : 1;
    P.pel = bw->nPel; P.logPel = bw->nPel == 4 ? 2 : bw->nPel == 2 ? 1 : 0;
    P.bits = si.bits; P.bps = (si.bits + 7) / 8;
    P.nBlkX = bw->nBlkX; P.nBlkY = bw->nBlkY; P.nBlk = bw->nBlkX * bw->nBlkY; P.nLvCount = bw->nLvCount;
    P.stepX = bw->nBlkSizeX - bw->nOverlapX; P.stepY = bw->nBlkSizeY - bw->nOverlapY;
    P.XP = bw->nBlkX; P.YP = bw->nBlkY;
    if (padded) fps_padded_grid(bw, &P.XP, &P.YP, nWidthP, nHeightP);
    else {
        nWidthP[0] = bw->nWidth; nHeightP[0] = bw->nHeight;
        nWidthP[1] = bw->nWidth / bw->xRatioUV; nHeightP[1] = bw->nHeight / bw->yRatioUV;
    }
    P.limW[0] = bw->nWidth; P.limH[0] = bw->nHeight;
    P.limW[1] = bw->nWidth / bw->xRatioUV; P.limH[1] = bw->nHeight / bw->yRatioUV;
    P.halfX = bw->xRatioUV == 2; P.halfY = bw->yRatioUV == 2;
    // the upsizer interpolates between small-field cells o and o + 1: with a single (padded) column or row the reference reads outside its buffers
    if (P.XP < 2 || P.YP < 2) MVX_FAIL("%s: the frame must be at least two blocks wide and two blocks high.", name);
    if (si.num_planes > 1 && super_pitch[1] != super_pitch[2]) MVX_FAIL("%s: U and V super planes must share one pitch.", name);
    fps_fill_planes(P.pl, bw, si, nullptr, super_pitch, dst_pitch);
    // the plane layouts (mvx_fps_shared.h), prefixed with the filter's name like every message of the flow filters
    char msg[MVX_ERRLEN];
    if (fps_check_super_pitches(si, super_pitch, msg) || fps_check_pitches("clip", P.pl, P.nplanes, clip_pitch, P.bps, msg) ||
        fps_check_pitches("dst", P.pl, P.nplanes, dst_pitch, P.bps, msg)) MVX_FAIL("%s: %s", name, msg);
    for (int p = 0; p < 3; p++) P.clipPitch[p] = clip_pitch[p < si.num_planes ? p : 0];
    return MVX_OK;
}

// FlowInter / FlowFPS: the two-clip checks, then the padded geometry.  The integer entries say the geometry's and the pitches' messages before
// their frame-size checks (`sizes`); the float entries (flt) say the reference's messages in the reference's order first, then that the
// super clip is no float one, then the library's own
template <typename SIZES>
static int flow_common(mvx_flow *h, const char *name, int64_t arg1, int32_t arg2, const mvx_analysis_data *bw, const mvx_analysis_data *fw, const mvx_super *sup,
                       const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], bool flt, char *err, SIZES &&sizes) {
    const mvx_super_info &si = sup->info;
    int64_t thscd1; int32_t thscd2;
    if (int rc = flow_pair_checks(name, arg1, arg2, &thscd1, &thscd2, bw, fw, err)) return rc;
    if (flt) {
        if (int rc = sizes()) return rc;
        if (!sup->is_float) MVX_FAIL("%s: the float entry needs a float super clip.", name);
    }
    if (int rc = flow_geometry(h->P, h->nWidthP, h->nHeightP, name, thscd1, thscd2, bw, si, super_pitch, clip_pitch, dst_pitch, true, err)) return rc;
    if (!flt)
        if (int rc = sizes()) return rc;
    h->delta = bw->nDeltaFrame;
    return MVX_OK;
}

// the luma / chroma launches of a kernel that produces CW consecutive samples per thread, the widest segment that divides the plane width (the
// tables cover nWidthP >= the width): go(grid, first plane, planes per job, fps_type<T>, integral constant CW).  Every kernel of this file
// that takes it also runs on float32 samples (T = float: segments of 4, 2 or 1 samples)
template <typename F> static void fm_launches(const FLParams &P, int nframes, F &&go) {
    fps_classes(P.pl, P.nplanes, nframes, [&](int p) { return fps_segment(P.bps, P.pl[p].W); }, [&](dim3 grid, int cw, int p0, int npl) {
        auto one = [&](auto t, auto w) { go(grid, p0, npl, t, w); };
        if (P.bps == 4) fps_dispatch_float<1>(cw, one); else fps_dispatch<1>(P.bps, cw, one);
    });
}

// MVFlowInter.c:473-678 mvflowinterCreate.  time and ml are float arguments there: time256 is formed in float, ml reaches the mask as (double)(float)ml.
// flt: the float entry (the super clip must be a float one; said after the frame-size check)
static int flowinter_create(const mvx_flowinter_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw, const mvx_super *sup, int num_frames,
                            const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flow **out, char *err, bool flt) {
    MVX_CREATE_BEGIN(out);
    if (!flt) MVX_REFUSE_FLOAT(sup, "FlowInter");
    const mvx_super_info &si = sup->info;
    const float time = (float)a->time, ml = (float)a->ml;
    const int blend = a->blend == MVX_UNSET ? 1 : !!a->blend;
    if (time < 0.0f || time > 100.0f) MVX_FAIL("FlowInter: time must be between 0 and 100 %% (inclusive).");
    if (ml <= 0.0f) MVX_FAIL("FlowInter: ml must be greater than 0.");
    mvx_flow *h = new mvx_flow();
    const int rc = flow_common(h, "FlowInter", a->thscd1, a->thscd2, bw, fw, sup, super_pitch, clip_pitch, dst_pitch, flt, err, [&]() -> int {
        if (!mvx_super_fits(bw, si, false)) MVX_FAIL("FlowInter: wrong source or super clip frame size.");
        return MVX_OK;
    });
    if (rc) { delete h; return rc; }
    FLParams &P = h->P;
    P.isFPS = 0; P.blend = blend; P.ml = (double)ml;
    h->time256 = (int)(time * 256.0f / 100.0f);
    h->rate = FpsRate();
    h->rate.outFrames = num_frames;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) int mvx_flowinter_create(const mvx_flowinter_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flow **out, char *err) {
    return flowinter_create(a, bw, fw, sup, num_frames, super_pitch, clip_pitch, dst_pitch, out, err, false);
}
extern "C" __attribute__((visibility("default"))) int mvx_flowinter_create_float(const mvx_flowinter_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flow **out, char *err) {
    return flowinter_create(a, bw, fw, sup, num_frames, super_pitch, clip_pitch, dst_pitch, out, err, true);
}

// MVFlowFPS.c:565-802 mvflowfpsCreate.  flt: the float entry, as above
static int flowfps_create(const mvx_flowfps_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw, const mvx_super *sup, int num_frames,
                          int64_t fps_num, int64_t fps_den, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3],
                          mvx_flow **out, char *err, bool flt) {
    MVX_CREATE_BEGIN(out);
    if (!flt) MVX_REFUSE_FLOAT(sup, "FlowFPS");
    const mvx_super_info &si = sup->info;
    const int mask = a->mask == MVX_UNSET ? 2 : a->mask;
    const int blend = a->blend == MVX_UNSET ? 1 : !!a->blend;
    if (mask < 0 || mask > 2) MVX_FAIL("FlowFPS: mask must be 0, 1, or 2.");
    if (a->ml <= 0.0) MVX_FAIL("FlowFPS: ml must be greater than 0.");
    mvx_flow *h = new mvx_flow();
    const int rc = flow_common(h, "FlowFPS", a->thscd1, a->thscd2, bw, fw, sup, super_pitch, clip_pitch, dst_pitch, flt, err, [&]() -> int {
        if (fps_num == 0 || fps_den == 0) MVX_FAIL("FlowFPS: The input clip must have a frame rate. Invoke AssumeFPS if necessary.");
        if (bw->nWidth != si.width || bw->nHeight != si.height) MVX_FAIL("FlowFPS: inconsistent source and vector frame size.");
        if (!mvx_super_fits(bw, si, false)) MVX_FAIL("FlowFPS: wrong source or super clip frame size.");
        if (!(bw->nWidth + bw->nHPadding * 2 == si.super_width && bw->nHeight + bw->nVPadding * 2 <= si.super_height))
            MVX_FAIL("FlowFPS: inconsistent clips frame size! Incomprehensible error messages are the best, right?");
        return MVX_OK;
    });
    if (rc) { delete h; return rc; }
    FLParams &P = h->P;
    P.isFPS = 1; P.maskmode = mask; P.blend = blend; P.ml = a->ml;
    fps_rate_init(h->rate, a->num, a->den, fps_num, fps_den, num_frames);
    h->time256 = 0;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) int mvx_flowfps_create(const mvx_flowfps_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, int64_t fps_num, int64_t fps_den, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3],
        const ptrdiff_t dst_pitch[3], mvx_flow **out, char *err) {
    return flowfps_create(a, bw, fw, sup, num_frames, fps_num, fps_den, super_pitch, clip_pitch, dst_pitch, out, err, false);
}
extern "C" __attribute__((visibility("default"))) int mvx_flowfps_create_float(const mvx_flowfps_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, int64_t fps_num, int64_t fps_den, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3],
        const ptrdiff_t dst_pitch[3], mvx_flow **out, char *err) {
    return flowfps_create(a, bw, fw, sup, num_frames, fps_num, fps_den, super_pitch, clip_pitch, dst_pitch, out, err, true);
}

extern "C" __attribute__((visibility("default"))) void mvx_flow_destroy(mvx_flow *h) { delete h; }
extern "C" __attribute__((visibility("default"))) void mvx_flow_get_info(const mvx_flow *h, mvx_flow_info *info) {
    info->num_frames = h->rate.outFrames; info->fps_num = h->rate.outNum; info->fps_den = h->rate.outDen;
}
// FlowInter: n -> (n, n + delta, time256) (MVFlowInter.c:86-100); FlowFPS: MVFlowFPS.c:92-99,125-134 (BlockFPS's arithmetic)
extern "C" __attribute__((visibility("default"))) void mvx_flow_map(const mvx_flow *h, int n, int *nleft, int *nright, int *time256) {
    if (!h->P.isFPS) { *nleft = n; *nright = n + h->delta; *time256 = h->time256; return; }
    fps_rate_map(h->rate, h->delta, n, nleft, nright, time256);
}

extern "C" __attribute__((visibility("default"))) int mvx_flow_frames(mvx_flow *h, int nframes, const mvx_flow_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    FLParams &P = h->P;
    for (int f = 0; f < nframes; f++) { // the jobs' checks, before anything is uploaded or launched
        const mvx_flow_job &s = jobs[f];
        if (s.time256 < 0 || s.time256 > 256) { mvx_set_error("mvx_flow_frames: time256 must be between 0 and 256"); return MVX_E_ARG; }
        const int copy = P.isFPS && s.time256 <= 0 ? 1 : P.isFPS && s.time256 >= 256 ? 2 : 0;
        const bool right = copy == 2 || (!copy && P.blend);
        if (!s.dst[0] || !s.clip_left[0] || (right && !s.clip_right[0])) { mvx_set_error("mvx_flow_frames: dst / clip_left / clip_right are required"); return MVX_E_ARG; }
        if (int rc = fps_check_planes("mvx_flow_frames", "dst", s.dst, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_flow_frames", "clip_left", s.clip_left, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_flow_frames", "clip_right", s.clip_right, P.nplanes, P.bps, right)) return rc;
        if (int rc = fps_check_planes("mvx_flow_frames", "super_left", s.super_left, P.nplanes, 16, false)) return rc;
        if (int rc = fps_check_planes("mvx_flow_frames", "super_right", s.super_right, P.nplanes, 16, false)) return rc;
    }
    CallGuard::Scope scope(h->guard, st);
    if (!h->dP.p) // MVFlowInter.c:677-679
        if (int rc = fps_upload_tables(h->dTables, h->dP, P, h->nWidthP, h->nHeightP)) return rc;
    const size_t n = (size_t)nframes, cellsN = (size_t)P.XP * P.YP;
    HIP_CHECK(h->dJobs.reserve(n));
    HIP_CHECK(h->dFlags.reserve(n * 4));
    HIP_CHECK(h->dSmall.reserve(n * 2 * cellsN));
    HIP_CHECK(h->dCells.reserve(n * cellsN));
    HIP_CHECK(h->dMasks.reserve(n * 2 * cellsN));
    std::vector<FLJob> hj(nframes);
    for (int f = 0; f < nframes; f++) {
        FLJob &j = hj[f];
        const mvx_flow_job &s = jobs[f];
        memset(&j, 0, sizeof(j));
        for (int p = 0; p < 3; p++) {
            j.supL[p] = (const unsigned char *)s.super_left[p]; j.supR[p] = (const unsigned char *)s.super_right[p];
            j.clipL[p] = (const unsigned char *)s.clip_left[p]; j.clipR[p] = (const unsigned char *)s.clip_right[p];
            j.dst[p] = (unsigned char *)s.dst[p];
        }
        j.blobF = (const unsigned char *)s.blob_fw; j.blobB = (const unsigned char *)s.blob_bw;
        j.blobFF = (const unsigned char *)s.blob_fw_extra; j.blobBB = (const unsigned char *)s.blob_bw_extra;
        j.time256 = s.time256;
        if (P.isFPS && s.time256 <= 0) j.copy = 1;
        else if (P.isFPS && s.time256 >= 256) j.copy = 2;
    }
    HIP_CHECK(hipMemcpyAsync(h->dJobs.p, hj.data(), sizeof(FLJob) * nframes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(flow_usable_kernel, dim3(nframes, 4), dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p);
    HIP_CHECK(hipMemsetAsync(h->dSmall.p, 0, n * 2 * cellsN * sizeof(int), st));
    hipLaunchKernelGGL(flow_occ_kernel, dim3((P.nBlk + 255) / 256, 2, nframes), dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, h->dSmall.p);
    hipLaunchKernelGGL(flow_cells_kernel, dim3((unsigned)((cellsN + 255) / 256), nframes), dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, h->dSmall.p, h->dCells.p, h->dMasks.p);
    fm_launches(P, nframes, [&](dim3 grid, int p0, int npl, auto t, auto w) { // (float32 planes as well)
        hipLaunchKernelGGL((flow_kernel<typename decltype(t)::type, decltype(w)::value>), grid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, h->dCells.p, h->dMasks.p, p0, npl);
    });
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}

// ================================================================================================ mv.Flow and mv.FlowBlur
//
// Both stand on the machinery above: usability per blob, int16 small-field cells, the int16 upsizer evaluated at each sample (fl_vup with
// the upsizer tables of fps_upload_tables) and reads from the super frame as if it were the Finest frame (fl_fetch).  Flow builds the padded
// fields of FlowInter (MVFlow.cpp:535-562) with field_shift added to every VY cell before the chroma halving (:264-302); FlowBlur builds
// unpadded fields and tables that end at the frame (MVFlowBlur.c:525-536).  A job whose vectors are unusable copies its clip frame.
//   fm_usable_kernel   : per (job, blob) -> usable flags
//   fm_cells_kernel    : per (job, cell) -> one packed int16 pair (vx low, vy high) per vector field
//   flowcomp_kernel    : Flow mode 0 (fetch), per CW consecutive samples -> one fetch per sample, one wide store
//   flowshift_scatter  : Flow mode 1 (shift), per CW consecutive source samples -> a 64-bit atomicMax of ((raster index + 1) << 16) | sample
//                        into the destination's winner; the last writer in raster order has the largest key, whatever the arrival order
//   flowshift_resolve  : per CW samples -> the winner's sample, or pixel_max where nobody wrote (the reference's memset)
//   flowblur_kernel    : per sample -> the data-dependent F and B tap loops of RealFlowBlur
// Each of the last four runs as one launch for the luma planes of all jobs and one for both chroma planes of all jobs.
//
// T = float (mvx_flowcomp_create_float, mvx_flowblur_create_float; the rules are in include/mvtools_amd.h): everything above the sample is the
// integer filter's -- usability, cells, the upsizer, time256 / blur256 / prec, tap counts and positions.  Flow only moves samples, so its
// kernels carry the 32 bits of each (fl_load / fl_fetch / fl_store) in segments of 4, 2 or 1 samples; the shift's key holds them whole, as
// ((raster index + 1) << 32) | bits, and a hole becomes 1.0f on luma and 0.5f on chroma.  FlowBlur adds the taps to a float32 sum one by one
// in the integer kernel's order and divides once.
struct FMJob {
    const unsigned char *sup[3];   // Flow: super frame nref; FlowBlur: super frame n; NULL = copy the clip frame
    const unsigned char *blob[2];  // Flow: vectors at n; FlowBlur: mvbw at n - delta, mvfw at n + delta
    const unsigned char *clip[3];
    unsigned char *dst[3];
    int fieldShift, pad;
};
struct FMWin { unsigned long long *win; long long job, off[3]; }; // Flow shift: winners per job and plane, W x H samples each

// Fakery.c:52-58,103-107,144-146 fgopIsUsable per (job, blob) -> flags[job][2]; a blob past nb counts as usable
__global__ __launch_bounds__(256) void fm_usable_kernel(const FLParams *Pp, const FMJob *jobs, int nb, int *flags) {
    const FLParams &P = *Pp;
    const int f = blockIdx.x, k = blockIdx.y;
    const FMJob &J = jobs[f];
    const unsigned char *blob = k < nb ? J.blob[k] : nullptr;
    const bool ok = fps_block_usable(blob, J.sup[0] && blob, P.nLvCount, P.nBlk, P.thscd1, P.thscd2);
    if (threadIdx.x == 0) flags[f * 2 + k] = k >= nb || ok;
}
__device__ __forceinline__ bool fm_ok(const int *flags, int f) { return flags[2 * f] && flags[2 * f + 1]; }

// MakeVectorSmallMasks into the XP x YP grid (CheckAndPadSmallY where XP / YP exceed the block grid), then VY += fieldShift on every cell
__global__ __launch_bounds__(256) void fm_cells_kernel(const FLParams *Pp, const FMJob *jobs, int nb, const int *flags, int *cells) {
    const FLParams &P = *Pp;
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int cellsN = P.XP * P.YP;
    if (!fm_ok(flags, f) || i >= cellsN) return;
    const FMJob &J = jobs[f];
    const int y = i / P.XP, x = i - y * P.XP;
    const int sb = min(x, P.nBlkX - 1) + min(y, P.nBlkY - 1) * P.nBlkX;
    for (int k = 0; k < nb; k++) {
        short vx, vy;
        fl_padded(mvx_level0(J.blob[k], P.nLvCount), sb, x >= P.nBlkX, y >= P.nBlkY, vx, vy);
        vy = (short)(vy + J.fieldShift);
        cells[((size_t)f * cellsN + i) * nb + k] = (int)(unsigned short)vx | ((int)vy << 16);
    }
}

// the upsized vector of field k at one sample: vx, vy with the int16 resizer's limits, chroma halving by >> hx / hy on the cells
struct FMAt {
    int wt, wb, r0, r1, hx, hy, yLo, yHi;
    __device__ __forceinline__ void vec(DG_GL const unsigned char *cl, int nb, int k, int o, int wl, int wr, int xLo, int xHi, int &vx, int &vy) const {
        const int a0 = *(DG_GL const int *)(cl + 4 * ((r0 + o) * nb + k)), b0 = *(DG_GL const int *)(cl + 4 * ((r0 + o + 1) * nb + k));
        const int a1 = *(DG_GL const int *)(cl + 4 * ((r1 + o) * nb + k)), b1 = *(DG_GL const int *)(cl + 4 * ((r1 + o + 1) * nb + k));
        vx = fl_vup(fl_lo(a0) >> hx, fl_lo(a1) >> hx, fl_lo(b0) >> hx, fl_lo(b1) >> hx, wt, wb, wl, wr, xLo, xHi);
        vy = fl_vup(fl_hi(a0) >> hy, fl_hi(a1) >> hy, fl_hi(b0) >> hy, fl_hi(b1) >> hy, wt, wb, wl, wr, yLo, yHi);
    }
};
__device__ __forceinline__ FMAt fm_at(const FLParams &P, int c, int y) {
    FMAt a;
    a.wb = *(DG_GL const int *)dg_gl(P.vW[c] + y); a.wt = 16384 - a.wb;
    a.r0 = *(DG_GL const int *)dg_gl(P.vOff[c] + y) * P.XP; a.r1 = a.r0 + P.XP;
    a.hx = c && P.halfX ? 1 : 0; a.hy = c && P.halfY ? 1 : 0;
    a.yLo = -y * P.pel; a.yHi = (P.limH[c] - y) * P.pel - 1;
    return a;
}

// the output samples x .. x + CW - 1 of row y of job f, plane p: the clip frame's, when the job copies
template <typename T, int CW>
__device__ __forceinline__ bool fm_copy(const FLParams &P, const FMJob &J, const int *flags, int f, int p, int x, int y, DG_GL unsigned char *dptr) {
    if (fm_ok(flags, f)) return false;
    int l[CW];
    fl_load<T, CW>(dg_gl(J.clip[p] + (long long)y * P.clipPitch[p] + (long long)x * (long long)sizeof(T)), l);
    fl_store<T, CW>(dptr, l);
    return true;
}

// MVFlow.cpp:93-116 flowFetch: v = (V * time256 + 128) >> 8, the sample Finest(nref)[(h << lp) + vy][(w << lp) + vx]
template <typename T, int CW>
__global__ __launch_bounds__(256) void flowcomp_kernel(const FLParams *Pp, const FMJob *jobs, const int *flags, const int *cells, int time256,
                                                       int planeFirst, int planesPerFrame) {
    const FLParams &P = *Pp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * CW, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const FMJob &J = jobs[f];
    DG_GL unsigned char *dptr = dg_glw(J.dst[p] + (long long)y * g.dstPitch + (long long)x * (long long)sizeof(T));
    if (fm_copy<T, CW>(P, J, flags, f, p, x, y, dptr)) return;
    const int c = p ? 1 : 0;
    const FMAt at = fm_at(P, c, y);
    int hO[CW], hWr[CW];
    dg_load_ints<CW>(dg_gl(P.hOff[c] + x), hO);
    dg_load_ints<CW>(dg_gl(P.hW[c] + x), hWr);
    DG_GL const unsigned char *cl = dg_gl(cells + (size_t)f * P.XP * P.YP);
    const int Y = y << P.logPel;
    int out[CW];
#pragma unroll
    for (int i = 0; i < CW; i++) {
        const int xi = x + i;
        int vx, vy;
        at.vec(cl, 1, 0, hO[i], 16384 - hWr[i], hWr[i], -xi * P.pel, (P.limW[c] - xi) * P.pel - 1, vx, vy);
        out[i] = fl_fetch<T>(P, g, J.sup[p], (xi << P.logPel) + ((vx * time256 + 128) >> 8), Y + ((vy * time256 + 128) >> 8));
    }
    fl_store<T, CW>(dptr, out);
}

// MVFlow.cpp:119-148 flowShift, the scatter: source sample (y, x) = Finest(nref)[y << lp][x << lp] (sub-plane 0 of the super frame, so
// CW of them are one wide load) goes to (y + vy, x + vx) with v = (-V * time256 + (128 << lp)) >> (8 + lp), when that lies inside the plane
template <typename T, int CW>
__global__ __launch_bounds__(256) void flowshift_scatter(const FLParams *Pp, const FMJob *jobs, const int *flags, const int *cells, int time256, FMWin w,
                                                         int planeFirst, int planesPerFrame) {
    const FLParams &P = *Pp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * CW, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H || !fm_ok(flags, f)) return;
    const FMJob &J = jobs[f];
    const int c = p ? 1 : 0;
    const FMAt at = fm_at(P, c, y);
    int hO[CW], hWr[CW], s[CW];
    dg_load_ints<CW>(dg_gl(P.hOff[c] + x), hO);
    dg_load_ints<CW>(dg_gl(P.hW[c] + x), hWr);
    fl_load<T, CW>(dg_gl(J.sup[p] + sup_offset(g, P.pel, P.logPel, (int)sizeof(T), x << P.logPel, y << P.logPel)), s);
    DG_GL const unsigned char *cl = dg_gl(cells + (size_t)f * P.XP * P.YP);
    DG_GL unsigned long long *win = (DG_GL unsigned long long *)(unsigned long long)(w.win + f * w.job + w.off[p]);
    const int lp = P.logPel, rounding = 128 << lp, shift = 8 + lp;
#pragma unroll
    for (int i = 0; i < CW; i++) {
        const int xi = x + i;
        int vx, vy;
        at.vec(cl, 1, 0, hO[i], 16384 - hWr[i], hWr[i], -xi * P.pel, (P.limW[c] - xi) * P.pel - 1, vx, vy);
        const int dx = xi + ((-vx * time256 + rounding) >> shift), dy = y + ((-vy * time256 + rounding) >> shift);
        if (dx >= 0 && dx < g.W && dy >= 0 && dy < g.H) {
            // float: the payload takes the low 32 bits and the index the high ones.  It fits them for every legal frame: a plane has
            // fewer than 2^32 samples, or the 32-bit byte offsets of sup_offset could not address its super plane
            unsigned long long key;
            if constexpr (sizeof(T) == 4) key = ((unsigned long long)((long long)y * g.W + xi + 1) << 32) | (unsigned)s[i];
            else key = ((unsigned long long)((long long)y * g.W + xi + 1) << 16) | (unsigned)s[i];
            __hip_atomic_fetch_max(win + (long long)dy * g.W + dx, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// MVFlow.cpp:312,336-337 + the scatter's result: the low 16 bits of the winner, pixel_max where no source landed.  Float: the low 32 bits,
// and the top of the plane's nominal range where no source landed -- 1.0f on luma, 0.5f on chroma, which is centred on 0
typedef unsigned long long fm_u64x2 __attribute__((ext_vector_type(2), aligned(8)));
template <typename T> __device__ __forceinline__ int fm_payload(unsigned long long k) {
    if constexpr (sizeof(T) == 4) return (int)(unsigned)k; else return (int)(k & 0xffff);
}
template <typename T> __device__ __forceinline__ int fm_hole(const FLParams &P, int p) {
    if constexpr (sizeof(T) == 4) return p ? 0x3f000000 : 0x3f800000; else return (1 << P.bits) - 1;
}
template <typename T, int CW>
__global__ __launch_bounds__(256) void flowshift_resolve(const FLParams *Pp, const FMJob *jobs, const int *flags, FMWin w, int planeFirst, int planesPerFrame) {
    const FLParams &P = *Pp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * CW, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const FMJob &J = jobs[f];
    DG_GL unsigned char *dptr = dg_glw(J.dst[p] + (long long)y * g.dstPitch + (long long)x * (long long)sizeof(T));
    if (fm_copy<T, CW>(P, J, flags, f, p, x, y, dptr)) return;
    DG_GL const unsigned long long *win = (DG_GL const unsigned long long *)(unsigned long long)(w.win + f * w.job + w.off[p] + (long long)y * g.W + x);
    const int pixel_max = fm_hole<T>(P, p);
    int out[CW];
    if constexpr (CW == 1) {
        const unsigned long long k = *win;
        out[0] = k ? fm_payload<T>(k) : pixel_max;
    } else {
#pragma unroll
        for (int i = 0; i < CW; i += 2) {
            const fm_u64x2 k = *(DG_GL const fm_u64x2 *)(win + i);
            out[i] = k[0] ? fm_payload<T>(k[0]) : pixel_max;
            out[i + 1] = k[1] ? fm_payload<T>(k[1]) : pixel_max;
        }
    }
    fl_store<T, CW>(dptr, out);
}

// MVFlowBlur.c:72-130 RealFlowBlur at one sample, F then B: m = (max(|v0x|, |v0y|) / prec) >> 8 taps at ((i + 1) * v0 >> 8) with
// v0 = V * blur256 / m (C's truncating division; >> is arithmetic), the mean of the sample and the taps.  Every tap lies inside the
// frame: the upsizer limits |V| to the frame, and |(i + 1) * v0| <= |V * blur256| with blur256 <= 256.  The sum stays int32 as in the
// reference: it holds 16-bit samples while mF + mB < 32767.
// Float: sum = s(X, Y), then sum = sum + tap in float32 for the F taps and the B taps in this order, each addition rounded on its own, and
// sum / (float)(mF + mB + 1) -- one division, no reciprocal, nothing to fuse, no clamp; without taps it is x / 1.0f, the sample itself.
template <typename T> struct fb_sum { typedef int type; static __device__ __forceinline__ int of(int s) { return s; } };
template <> struct fb_sum<float> { typedef float type; static __device__ __forceinline__ float of(int s) { return __int_as_float(s); } };
template <typename T>
__device__ __forceinline__ int fb_taps(const FLParams &P, const PlaneG &g, const unsigned char *sup, int X, int Y, int vx, int vy, int blur256, int prec,
                                       typename fb_sum<T>::type &sum) {
    int vx0 = vx * blur256, vy0 = vy * blur256;
    const int m = (max(abs(vx0), abs(vy0)) / prec) >> 8;
    if (m > 0) {
        vx0 /= m; vy0 /= m;
        int ax = vx0, ay = vy0;
        for (int i = 0; i < m; i++) {
            sum = sum + fb_sum<T>::of(fl_fetch<T>(P, g, sup, X + (ax >> 8), Y + (ay >> 8)));
            ax += vx0; ay += vy0;
        }
    }
    return m;
}
template <typename T>
__global__ __launch_bounds__(256) void flowblur_kernel(const FLParams *Pp, const FMJob *jobs, const int *flags, const int *cells, int blur256, int prec,
                                                       int planeFirst, int planesPerFrame) {
    const FLParams &P = *Pp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const FMJob &J = jobs[f];
    DG_GL unsigned char *dptr = dg_glw(J.dst[p] + (long long)y * g.dstPitch + (long long)x * (long long)sizeof(T));
    if (fm_copy<T, 1>(P, J, flags, f, p, x, y, dptr)) return;
    const int c = p ? 1 : 0;
    const FMAt at = fm_at(P, c, y);
    const int o = *(DG_GL const int *)dg_gl(P.hOff[c] + x), wr = *(DG_GL const int *)dg_gl(P.hW[c] + x);
    DG_GL const unsigned char *cl = dg_gl(cells + (size_t)f * P.XP * P.YP * 2);
    const int xLo = -x * P.pel, xHi = (P.limW[c] - x) * P.pel - 1;
    int vxB, vyB, vxF, vyF;
    at.vec(cl, 2, 0, o, 16384 - wr, wr, xLo, xHi, vxB, vyB);
    at.vec(cl, 2, 1, o, 16384 - wr, wr, xLo, xHi, vxF, vyF);
    const int X = x << P.logPel, Y = y << P.logPel;
    typename fb_sum<T>::type sum = fb_sum<T>::of(fl_fetch<T>(P, g, J.sup[p], X, Y));
    const int mF = fb_taps<T>(P, g, J.sup[p], X, Y, vxF, vyF, blur256, prec, sum);
    const int mB = fb_taps<T>(P, g, J.sup[p], X, Y, vxB, vyB, blur256, prec, sum);
    int out;
    if constexpr (sizeof(T) == 4) out = __float_as_int(sum / (float)(mF + mB + 1)); else out = sum / (mF + mB + 1);
    fl_store<T, 1>(dptr, &out);
}

// ------------------------------------------------------------------------------------------------ host objects

struct FMEngine {
    CallGuard guard;
    FLParams P;
    DevBuf<FLParams> dP;
    DevBuf<FMJob> dJobs;                         // the per-job buffers hold exactly the largest call's jobs
    DevBuf<int> dFlags, dCells, dTables;
    DevBuf<unsigned long long> dWin;
    int nWidthP[2], nHeightP[2];
    int nb = 1;                                  // vector fields per job: Flow 1, FlowBlur 2 (B, F)
    int numFrames = 0, delta = 0, isb = 0, mode = 0, fields = 0, time256 = 0, blur256 = 0, prec = 1;
    long long winJob = 0, winOff[3] = {0, 0, 0}; // Flow shift: winner samples per job, per plane offsets
};
struct mvx_flowcomp : FMEngine {};
struct mvx_flowblur : FMEngine {};

// the per-call part both filters share: buffers for nframes jobs, the job table, usability and the cells
static int fm_prologue(FMEngine *h, int nframes, const std::vector<FMJob> &hj, hipStream_t st) {
    FLParams &P = h->P;
    if (!h->dP.p)
        if (int rc = fps_upload_tables(h->dTables, h->dP, P, h->nWidthP, h->nHeightP)) return rc;
    const size_t n = (size_t)nframes, cellsN = (size_t)P.XP * P.YP;
    HIP_CHECK(h->dJobs.reserve(n));
    HIP_CHECK(h->dFlags.reserve(n * 2));
    HIP_CHECK(h->dCells.reserve(n * cellsN * h->nb));
    if (h->nb == 1 && h->mode == 1) HIP_CHECK(h->dWin.reserve(n * (size_t)h->winJob)); // Flow's shift mode
    HIP_CHECK(hipMemcpyAsync(h->dJobs.p, hj.data(), sizeof(FMJob) * nframes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fm_usable_kernel, dim3(nframes, 2), dim3(256), 0, st, h->dP.p, h->dJobs.p, h->nb, h->dFlags.p);
    hipLaunchKernelGGL(fm_cells_kernel, dim3((unsigned)((cellsN + 255) / 256), nframes), dim3(256), 0, st, h->dP.p, h->dJobs.p, h->nb, h->dFlags.p, h->dCells.p);
    return MVX_OK;
}

// the geometry part of creation (after each filter's own checks): the size check, then the grid.  not_float: a float entry was handed an
// integer super clip (said after the size check)
static int fm_create(FMEngine *h, const char *name, int64_t thscd1, int32_t thscd2, const mvx_analysis_data *ad, const mvx_super_info &si,
                     const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], bool padded, bool not_float, char *err) {
    if (!mvx_super_fits(ad, si, false)) MVX_FAIL("%s: wrong source or super clip frame size.", name);
    if (not_float) MVX_FAIL("%s: the float entry needs a float super clip.", name);
    if (int rc = flow_geometry(h->P, h->nWidthP, h->nHeightP, name, thscd1, thscd2, ad, si, super_pitch, clip_pitch, dst_pitch, padded, err)) return rc;
    long long o = 0;
    for (int p = 0; p < 3; p++) {
        h->winOff[p] = o;
        if (p < h->P.nplanes) o += (long long)h->P.pl[p].W * h->P.pl[p].H;
    }
    h->winJob = o;
    h->delta = ad->nDeltaFrame; h->isb = ad->isBackward;
    return MVX_OK;
}

// MVFlow.cpp:391-593 mvflowCreate.  time is a double argument there: time256 is formed in double (FlowInter forms it in float).
// flt: the float entry (the super clip must be a float one; said after the frame-size check.  fields = 1 is refused last)
static int flowcomp_create(const mvx_flowcomp_args *a, const mvx_analysis_data *vectors, const mvx_super *sup, int num_frames, const ptrdiff_t super_pitch[3],
                           const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowcomp **out, char *err, bool flt) {
    MVX_CREATE_BEGIN(out);
    if (!flt) MVX_REFUSE_FLOAT(sup, "Flow");
    const double time = a->time;
    const int mode = a->mode == MVX_UNSET ? 0 : a->mode;
    int64_t thscd1; int32_t thscd2;
    if (time < 0.0 || time > 100.0) MVX_FAIL("Flow: time must be between 0 and 100 %% (inclusive).");
    if (mode < 0 || mode > 1) MVX_FAIL("Flow: mode must be 0 or 1.");
    if (int rc = mvx_resolve_thscd("Flow", a->thscd1, a->thscd2, vectors, &thscd1, &thscd2, err)) return rc;
    mvx_flowcomp *h = new mvx_flowcomp();
    if (int rc = fm_create(h, "Flow", thscd1, thscd2, vectors, sup->info, super_pitch, clip_pitch, dst_pitch, true, flt && !sup->is_float, err)) { delete h; return rc; }
    h->nb = 1; h->mode = mode;
    h->fields = a->fields == MVX_UNSET ? 0 : !!a->fields;
    if (flt && h->fields) { delete h; MVX_FAIL("Flow: fields is not supported on float clips."); }
    h->time256 = (int)(time * 256.0 / 100.0);
    h->numFrames = num_frames;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) int mvx_flowcomp_create(const mvx_flowcomp_args *a, const mvx_analysis_data *vectors, const mvx_super *sup,
        int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowcomp **out, char *err) {
    return flowcomp_create(a, vectors, sup, num_frames, super_pitch, clip_pitch, dst_pitch, out, err, false);
}
extern "C" __attribute__((visibility("default"))) int mvx_flowcomp_create_float(const mvx_flowcomp_args *a, const mvx_analysis_data *vectors, const mvx_super *sup,
        int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowcomp **out, char *err) {
    return flowcomp_create(a, vectors, sup, num_frames, super_pitch, clip_pitch, dst_pitch, out, err, true);
}
extern "C" __attribute__((visibility("default"))) void mvx_flowcomp_destroy(mvx_flowcomp *h) { delete h; }
// MVFlow.cpp:170-176: the reference frame of output frame n
extern "C" __attribute__((visibility("default"))) int mvx_flowcomp_ref(const mvx_flowcomp *h, int n) {
    return h->delta > 0 ? (h->isb ? n + h->delta : n - h->delta) : -h->delta;
}

extern "C" __attribute__((visibility("default"))) int mvx_flowcomp_frames(mvx_flowcomp *h, int nframes, const mvx_flowcomp_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    FLParams &P = h->P;
    for (int f = 0; f < nframes; f++) { // the jobs' checks, before the call takes the handle's guard
        const mvx_flowcomp_job &s = jobs[f];
        if (!s.dst[0] || !s.clip[0]) { mvx_set_error("mvx_flowcomp_frames: dst / clip are required"); return MVX_E_ARG; }
        if (int rc = fps_check_planes("mvx_flowcomp_frames", "dst", s.dst, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_flowcomp_frames", "clip", s.clip, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_flowcomp_frames", "ref_super", s.ref_super, P.nplanes, 16, false)) return rc;
    }
    CallGuard::Scope scope(h->guard, st);
    std::vector<FMJob> hj(nframes);
    for (int f = 0; f < nframes; f++) {
        FMJob &j = hj[f];
        const mvx_flowcomp_job &s = jobs[f];
        memset(&j, 0, sizeof(j));
        const bool comp = s.ref_super[0] && s.blob;
        for (int p = 0; p < 3; p++) {
            j.sup[p] = comp ? (const unsigned char *)s.ref_super[p] : nullptr;
            j.clip[p] = (const unsigned char *)s.clip[p]; j.dst[p] = (unsigned char *)s.dst[p];
        }
        j.blob[0] = comp ? (const unsigned char *)s.blob : nullptr;
        j.fieldShift = s.field_shift;
    }
    if (int rc = fm_prologue(h, nframes, hj, st)) return rc;
    if (h->mode == 0) {
        fm_launches(P, nframes, [&](dim3 grid, int p0, int npl, auto t, auto w) {
            hipLaunchKernelGGL((flowcomp_kernel<typename decltype(t)::type, decltype(w)::value>), grid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, h->dCells.p, h->time256, p0, npl);
        });
    } else {
        const FMWin win = { h->dWin.p, h->winJob, { h->winOff[0], h->winOff[1], h->winOff[2] } };
        HIP_CHECK(hipMemsetAsync(h->dWin.p, 0, (size_t)nframes * h->winJob * sizeof(unsigned long long), st));
        fm_launches(P, nframes, [&](dim3 grid, int p0, int npl, auto t, auto w) {
            hipLaunchKernelGGL((flowshift_scatter<typename decltype(t)::type, decltype(w)::value>), grid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, h->dCells.p, h->time256, win, p0, npl);
        });
        fm_launches(P, nframes, [&](dim3 grid, int p0, int npl, auto t, auto w) {
            hipLaunchKernelGGL((flowshift_resolve<typename decltype(t)::type, decltype(w)::value>), grid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, win, p0, npl);
        });
    }
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}

// MVFlowBlur.c:346-552 mvflowblurCreate.  blur is a float argument there: blur256 is formed in float.
// flt: the float entry (the super clip must be a float one; said after the frame-size check)
static int flowblur_create(const mvx_flowblur_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw, const mvx_super *sup, int num_frames,
                           const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowblur **out, char *err, bool flt) {
    MVX_CREATE_BEGIN(out);
    if (!flt) MVX_REFUSE_FLOAT(sup, "FlowBlur");
    const float blur = (float)a->blur;
    const int prec = a->prec == MVX_UNSET ? 1 : a->prec;
    int64_t thscd1; int32_t thscd2;
    if (blur < 0.0f || blur > 200.0f) MVX_FAIL("FlowBlur: blur must be between 0 and 200 %% (inclusive).");
    if (prec < 1) MVX_FAIL("FlowBlur: prec must be at least 1.");
    if (int rc = flow_pair_checks("FlowBlur", a->thscd1, a->thscd2, &thscd1, &thscd2, bw, fw, err)) return rc;
    mvx_flowblur *h = new mvx_flowblur();
    if (int rc = fm_create(h, "FlowBlur", thscd1, thscd2, bw, sup->info, super_pitch, clip_pitch, dst_pitch, false, flt && !sup->is_float, err)) { delete h; return rc; }
    h->nb = 2; h->prec = prec;
    h->blur256 = (int)(blur * 256.0f / 200.0f);
    h->numFrames = num_frames;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) int mvx_flowblur_create(const mvx_flowblur_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowblur **out,
        char *err) {
    return flowblur_create(a, bw, fw, sup, num_frames, super_pitch, clip_pitch, dst_pitch, out, err, false);
}
extern "C" __attribute__((visibility("default"))) int mvx_flowblur_create_float(const mvx_flowblur_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowblur **out,
        char *err) {
    return flowblur_create(a, bw, fw, sup, num_frames, super_pitch, clip_pitch, dst_pitch, out, err, true);
}
extern "C" __attribute__((visibility("default"))) void mvx_flowblur_destroy(mvx_flowblur *h) { delete h; }

extern "C" __attribute__((visibility("default"))) int mvx_flowblur_frames(mvx_flowblur *h, int nframes, const mvx_flowblur_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    FLParams &P = h->P;
    for (int f = 0; f < nframes; f++) { // the jobs' checks, before the call takes the handle's guard
        const mvx_flowblur_job &s = jobs[f];
        if (!s.dst[0] || !s.clip[0]) { mvx_set_error("mvx_flowblur_frames: dst / clip are required"); return MVX_E_ARG; }
        if (int rc = fps_check_planes("mvx_flowblur_frames", "dst", s.dst, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_flowblur_frames", "clip", s.clip, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_flowblur_frames", "super", s.super, P.nplanes, 16, false)) return rc;
    }
    CallGuard::Scope scope(h->guard, st);
    std::vector<FMJob> hj(nframes);
    for (int f = 0; f < nframes; f++) {
        FMJob &j = hj[f];
        const mvx_flowblur_job &s = jobs[f];
        memset(&j, 0, sizeof(j));
        const bool comp = s.super[0] && s.blob_bw && s.blob_fw;
        for (int p = 0; p < 3; p++) {
            j.sup[p] = comp ? (const unsigned char *)s.super[p] : nullptr;
            j.clip[p] = (const unsigned char *)s.clip[p]; j.dst[p] = (unsigned char *)s.dst[p];
        }
        j.blob[0] = comp ? (const unsigned char *)s.blob_bw : nullptr;
        j.blob[1] = comp ? (const unsigned char *)s.blob_fw : nullptr;
    }
    if (int rc = fm_prologue(h, nframes, hj, st)) return rc;
    fps_classes(P.pl, P.nplanes, nframes, [](int) { return 1; }, [&](dim3 grid, int, int p0, int npl) { // one sample per thread
        if (P.bps == 4) hipLaunchKernelGGL((flowblur_kernel<float>), grid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, h->dCells.p, h->blur256, h->prec, p0, npl);
        else if (P.bps == 1) hipLaunchKernelGGL((flowblur_kernel<uint8_t>), grid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, h->dCells.p, h->blur256, h->prec, p0, npl);
        else hipLaunchKernelGGL((flowblur_kernel<uint16_t>), grid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dFlags.p, h->dCells.p, h->blur256, h->prec, p0, npl);
    });
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}
