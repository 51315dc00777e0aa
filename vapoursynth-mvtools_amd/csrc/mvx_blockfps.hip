// mvx_blockfps.hip -- mv.BlockFPS on gfx950, integer and float clips.
// MVBlockFPS.c:229-676 (frame), :741-1014 (creation); MaskFun.cpp:63-166,349-371; SimpleResize.cpp:27-121.
// One gather pass per output cell like Compensate: the two motion-compensated fetches (backward vectors at the left frame into the right
// super frame, forward vectors at the right frame into the left one, both scaled by the time position), the per-mode blend, the overlap
// window sum and ToPixels.  The occlusion / SAD masks live at block resolution (three small byte planes per frame pair) and are upsized
// bilinearly ON THE FLY per sample with the reference's integer tables, so no full-size mask planes exist.
//   usable kernel : per job          -> both vector fields valid and no scene change
//   mask kernels  : per (job, block) -> the small masks (modes 3..8)
//   plan kernel   : per (job, block) -> the byte offsets of the two compensated blocks inside the super planes
//   cell kernel   : per output cell  -> bf_cell_kernel<T, W, MODE>, one kernel for uint8_t, uint16_t and float samples and for every case
// What it shares with the other block filters is in mvx_block_shared.h, the float arithmetic in mvx_blockfps_float_rule.h.
#include "mvx_block_shared.h"
#include "mvx_blockfps_float_rule.h"

struct BFParams : BlkGeom {
    int mode, blend, XP, YP;            // padded small-mask grid
    int nWidthP[2], nHeightP[2];        // luma / chroma upsizer output sizes
    double ml;
    int supInterior[3];                 // byte offset of the un-padded level-0 sample (0,0) inside each super plane (:455-464)
    const int *hOff[2], *hW[2], *vOff[2], *vW[2]; // SimpleResize tables, luma / chroma
    long long clipPitch[3];
};
struct BFJob {
    const unsigned char *srcSup[3], *refSup[3]; // super frame nleft / nright
    const unsigned char *blobF, *blobB;         // mvfw vectors at nright, mvbw vectors at nleft
    const unsigned char *clipL[3], *clipR[3];
    unsigned char *dst[3];
    int time256, good;
};
struct BFPlan { unsigned offB[2], offF[2]; };    // luma / chroma offsets of the two compensated blocks

// per job: usable = both vector fields valid and no scene change (Fakery.c:144-146); 0 -> fallback
__global__ __launch_bounds__(256) void bf_usable_kernel(const BFParams *Pp, const BFJob *jobs, int *usable) {
    const BFParams &P = *Pp;
    const BFJob &J = jobs[blockIdx.x];
    const unsigned char *const blobs[2] = { J.blobF, J.blobB };
    const bool ok = fps_block_usable(blobs, J.good && J.time256 > 0 && J.time256 < 256, P.nLvCount, P.nBlk, P.thscd1, P.thscd2);
    if (threadIdx.x == 0) usable[blockIdx.x] = ok;
}

// small masks, pass 1: scatter-max (occlusion, MaskFun.cpp:91-130) or direct (SAD mask, :139-166) into int planes
// [job][F,B][YP*XP]; the scatter only ever takes maxima, so the order of the reference's loops does not matter.
__global__ __launch_bounds__(256) void bf_mask_kernel(const BFParams *Pp, const BFJob *jobs, const int *usable, int *small) {
    const BFParams &P = *Pp;
    const int f = blockIdx.z, dir = blockIdx.y; // dir 0 = forward mask, 1 = backward mask
    if (!usable[f] || P.mode < 3) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.nBlk) return;
    const BFJob &J = jobs[f];
    const GVecD *vec = mvx_level0((dir ? J.blobB : J.blobF), P.nLvCount);
    const int nBlkX = P.nBlkX, nBlkY = P.nBlkY, by = i / nBlkX, bx = i - by * nBlkX;
    const int time256 = dir ? 256 - J.time256 : J.time256;
    const int stepX = P.pl[0].stepX, stepY = P.pl[0].stepY, nPel = P.pel;
    int *m = small + ((size_t)f * 2 + dir) * P.XP * P.YP;
    if (P.mode <= 5) {
        fps_occlusion_block(vec, i, bx, by, nBlkX, nBlkY, dir, time256, stepX, stepY, nPel, P.ml, m, P.XP);
    } else {
        const int tX = (256 - time256) * 16 / (stepX * nPel), tY = (256 - time256) * 16 / (stepY * nPel);
        int bxi = bx - vec[i].x * tX / 4096, byi = by - vec[i].y * tY / 4096;
        if (bxi < 0 || bxi >= nBlkX || byi < 0 || byi >= nBlkY) { bxi = bx; byi = by; }
        const long long sad = vec[bxi + byi * nBlkX].sad >> (P.bits - 8);
        const double factor = 4.0 / (P.ml * P.pl[0].blkW * P.pl[0].blkH);
        const double l = 255 * ((double)sad * factor); // pow(x, 1.0) == x
        m[bx + by * P.XP] = (int)(unsigned char)((l > 255) ? 255 : l);
    }
}
// pass 2: byte planes [job][F,B,O][YP*XP] with the right / bottom padding clones (MaskFun.cpp:63-80) and O = F*B/255 (:93-101)
__global__ __launch_bounds__(256) void bf_mask_finish_kernel(const BFParams *Pp, const int *usable, const int *small, unsigned char *masks) {
    const BFParams &P = *Pp;
    const int f = blockIdx.y;
    if (!usable[f] || P.mode < 3) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.XP * P.YP) return;
    const int y = i / P.XP, x = i - y * P.XP;
    const int s = fps_pad_source(x, y, P.nBlkX, P.nBlkY, P.XP);
    const int *mF = small + ((size_t)f * 2 + 0) * P.XP * P.YP, *mB = small + ((size_t)f * 2 + 1) * P.XP * P.YP;
    const int vF = mF[s], vB = mB[s];
    unsigned char *o = masks + (size_t)f * 3 * P.XP * P.YP;
    o[i] = (unsigned char)vF;
    o[P.XP * P.YP + i] = (unsigned char)vB;
    o[2 * P.XP * P.YP + i] = (unsigned char)((vF * vB) / 255);
}

__global__ __launch_bounds__(256) void bf_plan_kernel(const BFParams *Pp, const BFJob *jobs, const int *usable, BFPlan *plan) {
    const BFParams &P = *Pp;
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.nBlk || !usable[f]) return;
    const BFJob &J = jobs[f];
    const int by = i / P.nBlkX, bx = i - by * P.nBlkX;
    const GVecD *vB = mvx_level0(J.blobB, P.nLvCount), *vF = mvx_level0(J.blobF, P.nLvCount);
    const int x = bx * P.pl[0].stepX, y = by * P.pl[0].stepY, t = J.time256; // FakeBlockData x / y, Fakery.c:31-32
    const int bX = x * P.pel + ((vB[i].x * (256 - t)) >> 8), bY = y * P.pel + ((vB[i].y * (256 - t)) >> 8);
    const int fX = x * P.pel + ((vF[i].x * t) >> 8), fY = y * P.pel + ((vF[i].y * t) >> 8);
    BFPlan r;
    for (int c = 0; c < 2; c++) { // the reference DIVIDES by the subsampling ratio here (:482-488), it does not shift
        const PlaneG &g = P.pl[c];
        const int xr = 1 << g.subX, yr = 1 << g.subY;
        r.offB[c] = sup_offset(g, P.pel, P.logPel, P.bps, bX / xr, bY / yr);
        r.offF[c] = sup_offset(g, P.pel, P.logPel, P.bps, fX / xr, fY / yr);
    }
    plan[(size_t)f * P.nBlk + i] = r;
}

// ---- what differs by sample type: the value of a sample, the blend of two frames, and the sum over overlapped blocks.
// uint8_t and uint16_t: the reference's integers, to the bit.  Every mode result is truncated to T before it is used, as RealResultBlock
// stores it into a block of T (MVBlockFPS.c:117-227); modes 1 and 2 truncate their inner blend as well.
template <typename T> struct BfRule {
    typedef int V;
    static __device__ __forceinline__ int of(unsigned bits) { return (int)bits; }
    static __device__ __forceinline__ unsigned bits(int v) { return (unsigned)v; }
    static __device__ __forceinline__ int median(int a, int b, int c) { const int mn = min(a, b), mx = max(a, b); return max(mn, min(mx, c)); }
    // Blend (MaskFun.cpp:349-371): `left` with weight 256 - t, `right` with weight t
    static __device__ __forceinline__ int time(int right, int left, int t) { return (int)(T)((left * (256 - t) + right * t) >> 8); }
    // mode: 0..5 (6, 7 and 8 compute like 3, 4 and 5); bits: the clip's depth
    static __device__ __forceinline__ int value(int mode, int bits, int t, int sVal, int rVal, int b, int fw, int mF, int mB, int mO) {
        int v;
        switch (mode) {
        case 0: v = (b * t + fw * (256 - t)) >> 8; break;
        case 1: v = median(rVal, sVal, (int)(T)((b * t + fw * (256 - t)) >> 8)); break;
        case 2: v = median((int)(T)((rVal * t + sVal * (256 - t)) >> 8), b, fw); break;
        case 3: v = (((mB * fw + (255 - mB) * b + 255) >> 8) * t + ((mF * b + (255 - mF) * fw + 255) >> 8) * (256 - t)) >> 8; break;
        case 4: {
            const int ff = (mF * b + (255 - mF) * fw + 255) >> 8, bb = (mB * fw + (255 - mB) * b + 255) >> 8;
            const int avg = (rVal * t + sVal * (256 - t) + 255) >> 8, m = (bb * t + ff * (256 - t)) >> 8;
            v = (avg * mO + m * (255 - mO) + 255) >> 8; break;
        }
        default: v = mO << (bits - 8); break;
        }
        return (int)(T)v;
    }
    struct Sum { // overlaps_c (Overlap.cpp:143-158) and ToPixels (:335-356)
        unsigned acc = 0;
        __device__ __forceinline__ void add(int v, int win) { acc += (unsigned)((v * win) >> 6); }
        __device__ __forceinline__ int out(int bits) const {
            const unsigned a0 = sizeof(T) == 1 ? acc & 0xffffu : acc; // 16-bit accumulator of the 8-bit path (Overlap.cpp:254-256)
            const int a = (int)((a0 + 16) >> 5), pm = (1 << bits) - 1;
            return a > pm ? pm : a;
        }
    };
};
// float: mvx_blockfps_float_rule.h
template <> struct BfRule<float> {
    typedef float V;
    static __device__ __forceinline__ float of(unsigned bits) { return __uint_as_float(bits); }
    static __device__ __forceinline__ unsigned bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float time(float right, float left, int t) { return mvx_bff_time(right, left, t); }
    static __device__ __forceinline__ float value(int mode, int, int t, float sVal, float rVal, float b, float fw, int mF, int mB, int mO) {
        return mvx_bff_value(mode, t, sVal, rVal, b, fw, mF, mB, mO);
    }
    struct Sum {
        float acc = 0.0f; int wsum = 0;
        __device__ __forceinline__ void add(float v, int win) { acc = mvx_bff_add(acc, v, win); wsum += win; }
        __device__ __forceinline__ float out(int) const { return mvx_bff_out(acc, wsum); }
    };
};

// ---- a cell's samples as they lie in memory (DgRaw): sample i as bits, and into a cell whose integer samples are still zero
template <typename T, int W> __device__ __forceinline__ unsigned bf_get(const DgRaw<T, W> &r, int i) {
    if constexpr (sizeof(T) == 4) return r.d[i]; else return (unsigned)dg_sample(r, i);
}
template <typename T, int W> __device__ __forceinline__ void bf_put(DgRaw<T, W> &r, int i, unsigned v) {
    if constexpr (sizeof(T) == 4) r.d[i] = v;
    else if constexpr (sizeof(T) == 2) r.d[i >> 1] |= v << (16 * (i & 1));
    else r.d[i >> 2] |= v << (8 * (i & 3));
}
// n: the samples of the cell inside the plane (W or more: all of them); a cell cut by the plane's edge is read and written sample by sample
template <typename T> struct BfMem { typedef T type; };
template <> struct BfMem<float> { typedef dg_uv1 type; }; // (float samples move as the bytes they are)
template <typename T, int W> __device__ __forceinline__ DgRaw<T, W> bf_load(DG_GL const unsigned char *p, int n) {
    if (n >= W) return dg_load_raw<T, W>(p);
    DgRaw<T, W> r = {};
#pragma unroll
    for (int i = 0; i < W; i++) bf_put(r, i, i < n ? (unsigned)*(DG_GL const typename BfMem<T>::type *)(p + sizeof(T) * i) : 0u);
    return r;
}
template <typename T, int W> __device__ __forceinline__ void bf_store(DG_GL unsigned char *p, const DgRaw<T, W> &r, int n) {
    constexpr int BYTES = W * (int)sizeof(T);
    if (n >= W) {
        if constexpr (BYTES == 16) { dg_uv4 t = { r.d[0], r.d[1], r.d[2], r.d[3] }; *(DG_GL dg_uv4 *)p = t; }
        else if constexpr (BYTES == 8) { dg_uv2 t = { r.d[0], r.d[1] }; *(DG_GL dg_uv2 *)p = t; }
        else if constexpr (BYTES == 4) *(DG_GL dg_uv1 *)p = r.d[0];
        else if constexpr (BYTES == 2) *(DG_GL dg_uh1 *)p = (unsigned short)r.d[0];
        else *p = (unsigned char)r.d[0];
        return;
    }
#pragma unroll
    for (int i = 0; i < W; i++) if (i < n) *(DG_GL typename BfMem<T>::type *)(p + sizeof(T) * i) = (typename BfMem<T>::type)bf_get(r, i);
}

// ---- the output kernel, of cn_cell_kernel<T, W>'s shape, for every case: overlapped blocks and blocks side by side, the copies and the blend
// of a job that is not usable, the strips no block covers, every mode.  A thread produces one row of a cell of W samples of T (16 bytes at
// most); 256 threads = 32 cells x 8 rows of one plane of one job.  W divides the block width and the block step (blk_cell_width), so the same
// <= 2 x 2 blocks cover all of a cell and each costs one vector load per fetch, and the covered width is a multiple of W: cells cut by the
// plane's right edge exist only in the fallback and in the strips.  Job, plane, geometry and tables are uniform over the workgroup and arrive
// through scalar loads.  The motion-compensated fetches are aligned to a sample and no more, as are the clip and the output planes.
// MODE: 0..5, the arithmetic of the mode (6, 7 and 8 compute like 3, 4 and 5: they differ in how the masks are made).  A template argument so
// that a mode keeps in registers only what it reads: 0..2 no mask, 3 F and B, 4 all three, 5 O alone and no fetch.  With the mode a run-time
// value every mode pays for mode 4's registers, integer samples too: 122 VGPRs against 95 for 8 8-bit samples in mode 3
// (profiles/blockfps_cell_isa.txt).  The masks of a sample travel packed in one register: F | B << 8 | O << 16
// The float mask modes divide two or three times per sample, and an IEEE division is a dozen instructions with half a dozen values in flight.
// Left alone the scheduler interleaves the divisions of all W samples (109 and 112 VGPRs at W = 4 in modes 3 and 4, occupancy 4); a scheduling
// barrier after each sample keeps one sample's temporaries live at a time (the integer mixes are shifts: it gains them nothing)
#define BF_ONE_AT_A_TIME() do { if constexpr (sizeof(T) == 4 && (MODE == 3 || MODE == 4)) __builtin_amdgcn_sched_barrier(0); } while (0)
template <typename T, int W, int MODE>
__global__ __launch_bounds__(256) void bf_cell_kernel(const BFParams P, const BFJob *jobs, const int *usable, const BFPlan *plan, const unsigned char *masks,
                                                      int planeFirst, int planesPerFrame) {
    typedef BfRule<T> Rule;
    static_assert(W * sizeof(T) <= 16, "cells of 16 bytes at most");
    const int z = blockIdx.z, p = planeFirst + (z & (planesPerFrame - 1)), f = z >> (planesPerFrame - 1); // (a class has one plane or two)
    const PlaneG &g = P.pl[p];
    const int x0 = (blockIdx.x * 32 + (threadIdx.x & 31)) * W, y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x0 >= g.W || y >= g.H) return;
    const int n = g.W - x0;
    const BFJob &J = jobs[f];
    DG_GL unsigned char *dptr = dg_glw(J.dst[p]) + (long long)y * g.dstPitch + (long long)x0 * (long long)sizeof(T);
    const int t = J.time256;
    DgRaw<T, W> out = {};
    if (!usable[f]) { // time256 0 / 256, vectors unusable or frames outside the clip (:285-288, :640-673): a copy, bit for bit, or the blend of the two clip frames
        const long long co = (long long)y * P.clipPitch[p] + (long long)x0 * (long long)sizeof(T);
        const bool left = t <= 0 || (t < 256 && !P.blend);
        if (left || t >= 256) { bf_store<T, W>(dptr, bf_load<T, W>(dg_gl(left ? J.clipL[p] : J.clipR[p]) + co, n), n); return; }
        const DgRaw<T, W> l = bf_load<T, W>(dg_gl(J.clipL[p]) + co, n), r = bf_load<T, W>(dg_gl(J.clipR[p]) + co, n);
#pragma unroll
        for (int i = 0; i < W; i++) bf_put(out, i, Rule::bits(Rule::time(Rule::of(bf_get(r, i)), Rule::of(bf_get(l, i)), t)));
        bf_store<T, W>(dptr, out, n);
        return;
    }
    const long long inner = P.supInterior[p] + (long long)y * g.supPitch + (long long)x0 * (long long)sizeof(T);
    const DgRaw<T, W> sVal = bf_load<T, W>(dg_gl(J.srcSup[p]) + inner, n), rVal = bf_load<T, W>(dg_gl(J.refSup[p]) + inner, n);
    const int covW = P.overlap ? g.WB : g.blkW * P.nBlkX, covH = P.overlap ? g.HB : g.blkH * P.nBlkY;
    if (x0 >= covW || y >= covH) { // Blend of the strips no block covers
#pragma unroll
        for (int i = 0; i < W; i++) bf_put(out, i, Rule::bits(Rule::time(Rule::of(bf_get(rVal, i)), Rule::of(bf_get(sVal, i)), t)));
        bf_store<T, W>(dptr, out, n);
        return;
    }
    // from here on the cell lies inside the covered width (a multiple of W), so inside the plane
    const int c = p ? 1 : 0;
    unsigned mk[W];
#pragma unroll
    for (int i = 0; i < W; i++) mk[i] = 0u;
    if constexpr (MODE >= 3) { // the upsizer (SimpleResize.cpp:62-121): the integer tables, the masks stay bytes.  Tables and mask bytes through
        // global-address-space pointers and as vectors: the table pointers sit in a struct, so the compiler would emit one flat load per entry
        DG_GL const unsigned char *m = dg_gl(masks + (size_t)f * 3 * P.XP * P.YP);
        const int wb = *(DG_GL const int *)dg_gl(P.vW[c] + y), wt = 16384 - wb;
        const int rowOff = *(DG_GL const int *)dg_gl(P.vOff[c] + y) * P.XP;
        int hO[W], hWr[W];
        dg_load_ints<W>(dg_gl(P.hOff[c] + x0), hO);
        dg_load_ints<W>(dg_gl(P.hW[c] + x0), hWr);
        const int o0 = hO[0];
        // vertically interpolated values of up to three mask columns; columns further right (upsizing by less than W) are done on demand
        auto vcol = [&](DG_GL const unsigned char *mm, int o) { return (int)(unsigned char)((mm[rowOff + o] * wt + mm[rowOff + P.XP + o] * wb + 8192) >> 14); };
        auto upsize = [&](DG_GL const unsigned char *mm, int shift) {
            // the bytes o0 .. o0 + 3 of the two mask rows as one unaligned dword each (the mask buffer has slack behind its last row); the third
            // column is only used when a sample's left neighbour is o0 + 1, and at the grid's right edge it does not exist: o0 + 1 again
            const unsigned r0 = *(DG_GL const dg_uv1 *)(mm + rowOff + o0), r1 = *(DG_GL const dg_uv1 *)(mm + rowOff + P.XP + o0);
            auto vc = [&](int k) { return (int)(unsigned char)((((r0 >> (8 * k)) & 0xffu) * wt + ((r1 >> (8 * k)) & 0xffu) * wb + 8192) >> 14); };
            const int a0 = vc(0), a1 = vc(1), a2 = o0 + 2 < P.XP ? vc(2) : a1;
#pragma unroll
            for (int i = 0; i < W; i++) {
                const int o = hO[i], wr = hWr[i], wl = 16384 - wr, k = o - o0;
                int a, b;
                if (k == 0) { a = a0; b = a1; } else if (k == 1) { a = a1; b = a2; } else { a = vcol(mm, o); b = vcol(mm, o + 1); }
                mk[i] |= (unsigned)(unsigned char)((a * wl + b * wr + 8192) >> 14) << shift;
            }
        };
        if constexpr (MODE != 5) { upsize(m, 0); upsize(m + P.XP * P.YP, 8); }
        if constexpr (MODE >= 4) upsize(m + 2 * P.XP * P.YP, 16);
    }
    // one sample of a block from its two fetches (RealResultBlock)
    auto value = [&](int i, const DgRaw<T, W> &bv, const DgRaw<T, W> &fv) {
        return Rule::value(MODE, P.bits, t, Rule::of(bf_get(sVal, i)), Rule::of(bf_get(rVal, i)), Rule::of(bf_get(bv, i)), Rule::of(bf_get(fv, i)), (int)(mk[i] & 0xffu),
                           (int)((mk[i] >> 8) & 0xffu), (int)(mk[i] >> 16));
    };
    DG_GL const unsigned char *pl = dg_gl(plan + (size_t)f * P.nBlk);
    DG_GL const unsigned char *refSup = dg_gl(J.refSup[p]), *srcSup = dg_gl(J.srcSup[p]);
    // the two fetches of block (bx, by) at the cell's (px, py) inside it; mode 5 reads neither
    auto fetch = [&](int bx, int by, int px, int py, DgRaw<T, W> &bv, DgRaw<T, W> &fv) {
        if constexpr (MODE != 5) {
            const dg_iv4 R = *(DG_GL const dg_iv4 *)(pl + (size_t)(by * P.nBlkX + bx) * sizeof(BFPlan));
            const long long bo = (long long)py * g.supPitch + (long long)px * (long long)sizeof(T);
            bv = dg_load_raw<T, W>(refSup + (unsigned)R[c] + bo);
            fv = dg_load_raw<T, W>(srcSup + (unsigned)R[2 + c] + bo);
        }
    };
    if (!P.overlap) { // blocks side by side (their sizes are powers of two: the host checks): the value itself
        DgRaw<T, W> bv = sVal, fv = sVal;
        const int lbw = __ffs(g.blkW) - 1, lbh = __ffs(g.blkH) - 1;
        fetch(x0 >> lbw, y >> lbh, x0 & (g.blkW - 1), y & (g.blkH - 1), bv, fv);
#pragma unroll
        for (int i = 0; i < W; i++) { bf_put(out, i, Rule::bits(value(i, bv, fv))); BF_ONE_AT_A_TIME(); }
        bf_store<T, W>(dptr, out, W);
        return;
    }
    // overlapped blocks: the blocks bx0..bx1 x by0..by1 cover the cell, at most two each way, by outer and bx inner.  One block at a time: its
    // two fetches and its window row are all that is live beside the cell's own state, which keeps the kernel at cn_cell_kernel<T, W>'s occupancy
    int bx0, bx1, by0, by1;
    blk_cover(x0, g.blkW, g.stepX, P.nBlkX, bx0, bx1);
    blk_cover(y, g.blkH, g.stepY, P.nBlkY, by0, by1);
    DG_GL const unsigned char *win = dg_gl(P.win[p]);
    typename Rule::Sum sum[W];
#pragma unroll 1
    for (int by = by0; by <= by1; by++) {
        const int py = y - by * g.stepY, wrow = BLK_WIN_ROW(by, P.nBlkY);
#pragma unroll 1
        for (int bx = bx0; bx <= bx1; bx++) {
            const int px = x0 - bx * g.stepX; // 0 <= px <= blkW - W
            DgRaw<T, W> bv = sVal, fv = sVal;
            fetch(bx, by, px, py, bv, fv);
            const DgRaw<unsigned short, W> wv = dg_load_raw<unsigned short, W>(win + (size_t)((wrow + BLK_WIN_COL(bx, P.nBlkX)) * g.blkW * g.blkH + py * g.blkW + px) * 2);
#pragma unroll
            for (int i = 0; i < W; i++) { sum[i].add(value(i, bv, fv), dg_sample(wv, i)); BF_ONE_AT_A_TIME(); }
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) bf_put(out, i, Rule::bits(sum[i].out(P.bits)));
    bf_store<T, W>(dptr, out, W);
}

struct mvx_blockfps {
    CallGuard guard;
    BFParams P;
    DevBuf<BFParams> dP;
    DevBuf<BFJob> dJobs;          // grows to twice the call's jobs, as do the usable flags, the plan and the masks
    DevBuf<int> dUsable;
    DevBuf<BFPlan> dPlan;
    BlkWin win;
    DevBuf<int> dSmall, dTables;
    DevBuf<unsigned char> dMasks;
    FpsRate rate;
    int delta;
    bool flt = false;             // float super clip, float clip and output planes
};

// MVBlockFPS.c:741-1014 mvblockfpsCreate.  flt: the float entry (the super clip must be a float one; said after the frame-size check)
static int bf_create(bool flt, const mvx_blockfps_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, int64_t fps_num, int64_t fps_den, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3],
        const ptrdiff_t dst_pitch[3], mvx_blockfps **out, char *err) {
    MVX_CREATE_BEGIN(out);
    if (!flt) MVX_REFUSE_FLOAT(sup, "BlockFPS");
    const mvx_super_info &si = sup->info;
    const int mode = a->mode == MVX_UNSET ? 3 : a->mode;
    const int blend = a->blend == MVX_UNSET ? 1 : !!a->blend;
    int64_t thscd1; int32_t thscd2;
    if (mode < 0 || mode > 8) MVX_FAIL("BlockFPS: mode must be between 0 and 8 (inclusive).");
    if (int rc = mvx_resolve_thscd("BlockFPS", a->thscd1, a->thscd2, bw, &thscd1, &thscd2, err)) return rc;
    // (the first mismatch is reported, and subsampling and bit depth are not compared: unlike flow_similarity in mvx_flow.hip)
    if (bw->nWidth != fw->nWidth) MVX_FAIL("BlockFPS: mvbw and mvfw have different widths.");
    if (bw->nHeight != fw->nHeight) MVX_FAIL("BlockFPS: mvbw and mvfw have different heights.");
    if (bw->nBlkSizeX != fw->nBlkSizeX || bw->nBlkSizeY != fw->nBlkSizeY) MVX_FAIL("BlockFPS: mvbw and mvfw have different block sizes.");
    if (bw->nPel != fw->nPel) MVX_FAIL("BlockFPS: mvbw and mvfw have different pel precision.");
    if (bw->nOverlapX != fw->nOverlapX || bw->nOverlapY != fw->nOverlapY) MVX_FAIL("BlockFPS: mvbw and mvfw have different overlap.");
    if (int rc = mvx_pair_checks("BlockFPS", bw, fw, err)) return rc;
    if (fps_num == 0 || fps_den == 0) MVX_FAIL("BlockFPS: The input clip must have a frame rate. Invoke AssumeFPS if necessary.");
    if (!mvx_super_fits(bw, si, true)) MVX_FAIL("BlockFPS: wrong source or super clip frame size.");
    if (flt && !sup->is_float) MVX_FAIL("BlockFPS: the float entry needs a float super clip.");
    mvx_blockfps *h;
    if (int rc = blk_new(&h, bw, si, clip_pitch, super_pitch, dst_pitch, err, "clip")) return rc;
    BFParams &P = h->P;
    h->flt = flt;
    // P.bps stays the sample size (4: pitches, the plan's offsets, supInterior).  P.bits is read by bf_mask_kernel alone on this path, as the
    // depth of the SADs (sad >> (bits - 8)): that of the search, not the super clip's 32
    if (flt) P.bits = bw->bitsPerSample;
    if (!(si.modeYUV & 6)) P.nplanes = 1;
    P.thscd1 = thscd1; P.thscd2 = thscd2;
    fps_rate_init(h->rate, a->num, a->den, fps_num, fps_den, num_frames);
    h->delta = bw->nDeltaFrame;
    P.mode = mode; P.blend = blend; P.ml = a->ml;
    fps_padded_grid(bw, &P.XP, &P.YP, P.nWidthP, P.nHeightP);
    const int bps = P.bps;
    P.supInterior[0] = si.hpad * bps + (int)super_pitch[0] * si.vpad;
    for (int p = 1; p < 3; p++) P.supInterior[p] = (si.hpad >> 1) * bps + (int)super_pitch[p < si.num_planes ? p : 0] * (si.vpad >> 1); // the reference's ">> 1" (:459-463)
    for (int p = 0; p < 3; p++) P.clipPitch[p] = clip_pitch[p < si.num_planes ? p : 0];
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) int mvx_blockfps_create(const mvx_blockfps_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, int64_t fps_num, int64_t fps_den, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3],
        const ptrdiff_t dst_pitch[3], mvx_blockfps **out, char *err) {
    return bf_create(false, a, bw, fw, sup, num_frames, fps_num, fps_den, super_pitch, clip_pitch, dst_pitch, out, err);
}
extern "C" __attribute__((visibility("default"))) int mvx_blockfps_create_float(const mvx_blockfps_args *a, const mvx_analysis_data *bw, const mvx_analysis_data *fw,
        const mvx_super *sup, int num_frames, int64_t fps_num, int64_t fps_den, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3],
        const ptrdiff_t dst_pitch[3], mvx_blockfps **out, char *err) {
    return bf_create(true, a, bw, fw, sup, num_frames, fps_num, fps_den, super_pitch, clip_pitch, dst_pitch, out, err);
}
extern "C" __attribute__((visibility("default"))) void mvx_blockfps_destroy(mvx_blockfps *b) { delete b; }
extern "C" __attribute__((visibility("default"))) void mvx_blockfps_get_info(const mvx_blockfps *b, mvx_blockfps_info *info) {
    info->num_frames = b->rate.outFrames; info->fps_num = b->rate.outNum; info->fps_den = b->rate.outDen;
}
extern "C" __attribute__((visibility("default"))) void mvx_blockfps_map(const mvx_blockfps *b, int n, int *nleft, int *nright, int *time256) {
    fps_rate_map(b->rate, b->delta, n, nleft, nright, time256);
}

// the cell kernel of w samples per cell, w a power of two up to WMAX: only the widths from WMAX down are instantiated
template <typename T, int MODE, int WMAX, typename... A> static void bf_launch(int w, dim3 grid, hipStream_t st, const A &...a) {
    if constexpr (WMAX > 1) { if (w < WMAX) return bf_launch<T, MODE, WMAX / 2>(w, grid, st, a...); }
    hipLaunchKernelGGL((bf_cell_kernel<T, WMAX, MODE>), grid, dim3(256), 0, st, a...);
}
// one launch for the luma planes of all jobs and one for both chroma planes, in mode m (0..5).  W0, W1, W4: the widest cell of the type in modes
// 0 and 5, in modes 1, 2 and 3, and in mode 4; a plane class takes the widest that divides its block width and block step (blk_cell_width)
template <typename T, int W0, int W1, int W4, typename... A> static void bf_launch_classes(const BFParams &P, int m, int nframes, hipStream_t st, const A &...a) {
    for (int cls = 0; cls < (P.nplanes > 1 ? 2 : 1); cls++) {
        const int p0 = cls, npl = cls ? 2 : 1, w = blk_cell_width(P.pl[p0], m == 0 || m == 5 ? W0 : m == 4 ? W4 : W1);
        const dim3 grid(((P.pl[p0].W + w - 1) / w + 31) / 32, (P.pl[p0].H + 7) / 8, nframes * npl);
        switch (m) {
        case 0: bf_launch<T, 0, W0>(w, grid, st, P, a..., p0, npl); break;
        case 1: bf_launch<T, 1, W1>(w, grid, st, P, a..., p0, npl); break;
        case 2: bf_launch<T, 2, W1>(w, grid, st, P, a..., p0, npl); break;
        case 3: bf_launch<T, 3, W1>(w, grid, st, P, a..., p0, npl); break;
        case 4: bf_launch<T, 4, W4>(w, grid, st, P, a..., p0, npl); break;
        default: bf_launch<T, 5, W0>(w, grid, st, P, a..., p0, npl); break;
        }
    }
}

extern "C" __attribute__((visibility("default"))) int mvx_blockfps_frames(mvx_blockfps *b, int nframes, const mvx_blockfps_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    BFParams &P = b->P;
    for (int f = 0; f < nframes; f++) {
        const mvx_blockfps_job &J = jobs[f];
        if (!J.clip_left[0] || (J.time256 > 0 && !J.clip_right[0])) { mvx_set_error("mvx_blockfps_frames: clip_left / clip_right are required"); return MVX_E_ARG; }
        if (int rc = fps_check_planes("mvx_blockfps_frames", "clip_left", J.clip_left, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_blockfps_frames", "clip_right", J.clip_right, P.nplanes, P.bps, false)) return rc;
        if (int rc = fps_check_planes("mvx_blockfps_frames", "dst", J.dst, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_blockfps_frames", "source super", J.src_super, P.nplanes, 16, false)) return rc;
        if (int rc = fps_check_planes("mvx_blockfps_frames", "reference super", J.ref_super, P.nplanes, 16, false)) return rc;
    }
    const int m = P.mode < 6 ? P.mode : P.mode - 3;
    // (the cell kernel finds a block among blocks side by side by shift and mask)
    for (int c = 0; c < (P.nplanes > 1 ? 2 : 1); c++)
        if (!P.overlap && ((P.pl[c].blkW & (P.pl[c].blkW - 1)) || (P.pl[c].blkH & (P.pl[c].blkH - 1)))) {
            mvx_set_error("mvx_blockfps_frames: blocks side by side must have power-of-two sizes");
            return MVX_E_ARG;
        }
    CallGuard::Scope scope(b->guard, st);
    if (!b->dP.p) { // the windows and the upsizer tables, then the parameter block, which points at both
        if (int rc = blk_upload_windows(P, b->win)) return rc;
        if (int rc = fps_upload_tables(b->dTables, b->dP, P, P.nWidthP, P.nHeightP)) return rc;
    }
    const size_t n = (size_t)nframes, cells = (size_t)P.XP * P.YP;
    HIP_CHECK(b->dJobs.reserve(n, n));
    HIP_CHECK(b->dUsable.reserve(n, n));
    HIP_CHECK(b->dPlan.reserve(n * P.nBlk, n * P.nBlk));
    HIP_CHECK(b->dSmall.reserve(n * 2 * cells, n * 2 * cells));
    HIP_CHECK(b->dMasks.reserve(n * 3 * cells + 16, n * 3 * cells)); // (+ slack: the cell kernel reads mask bytes four at a time)
    std::vector<BFJob> hj(nframes);
    for (int f = 0; f < nframes; f++) {
        BFJob &j = hj[f];
        memset(&j, 0, sizeof(j));
        for (int p = 0; p < 3; p++) {
            j.srcSup[p] = (const unsigned char *)jobs[f].src_super[p]; j.refSup[p] = (const unsigned char *)jobs[f].ref_super[p];
            j.clipL[p] = (const unsigned char *)jobs[f].clip_left[p]; j.clipR[p] = (const unsigned char *)jobs[f].clip_right[p];
            j.dst[p] = (unsigned char *)jobs[f].dst[p];
        }
        j.blobF = (const unsigned char *)jobs[f].blob_fw; j.blobB = (const unsigned char *)jobs[f].blob_bw;
        j.time256 = jobs[f].time256;
        j.good = j.srcSup[0] && j.refSup[0] && j.blobF && j.blobB;
    }
    HIP_CHECK(hipMemcpyAsync(b->dJobs.p, hj.data(), sizeof(BFJob) * nframes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bf_usable_kernel, dim3(nframes), dim3(256), 0, st, b->dP.p, b->dJobs.p, b->dUsable.p);
    if (P.mode >= 3) {
        HIP_CHECK(hipMemsetAsync(b->dSmall.p, 0, n * 2 * cells * sizeof(int), st));
        hipLaunchKernelGGL(bf_mask_kernel, dim3((P.nBlk + 255) / 256, 2, nframes), dim3(256), 0, st, b->dP.p, b->dJobs.p, b->dUsable.p, b->dSmall.p);
        hipLaunchKernelGGL(bf_mask_finish_kernel, dim3((unsigned)((cells + 255) / 256), nframes), dim3(256), 0, st, b->dP.p, b->dUsable.p, b->dSmall.p, b->dMasks.p);
    }
    hipLaunchKernelGGL(bf_plan_kernel, dim3((P.nBlk + 255) / 256, nframes), dim3(256), 0, st, b->dP.p, b->dJobs.p, b->dUsable.p, b->dPlan.p);
    // the widest cells by type and mode (profiles/blockfps_cell_isa.txt): integer samples 16 bytes, in modes 4 and 7 8 bytes -- the registers and
    // occupancy the row kernel had that this kernel replaced; float samples 16 bytes in modes 0, 5 and 8, 8 bytes in modes 1, 2, 3 and 6, one sample
    // in modes 4 and 7 -- occupancy 8
    const BFJob *dJ = b->dJobs.p; const int *dU = b->dUsable.p; const BFPlan *dPl = b->dPlan.p; const unsigned char *dM = b->dMasks.p;
    if (b->flt) bf_launch_classes<float, 4, 2, 1>(P, m, nframes, st, dJ, dU, dPl, dM);
    else if (P.bps == 1) bf_launch_classes<uint8_t, 16, 16, 8>(P, m, nframes, st, dJ, dU, dPl, dM);
    else bf_launch_classes<uint16_t, 8, 8, 4>(P, m, nframes, st, dJ, dU, dPl, dM);
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}
