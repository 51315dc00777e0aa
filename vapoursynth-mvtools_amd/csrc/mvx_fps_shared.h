// mvx_fps_shared.h -- device and host helpers shared by the block filters (mvx_degrain.hip) and the flow filters (mvx_flow.hip):
// the level-0 vector reader, the super-plane addressing, the wide sample loads / stores, the reference's bilinear upsizer tables and
// the occlusion mask of MaskFun.cpp.  Internal; not part of the ABI.
#pragma once
#include <algorithm>
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

// W samples of type T from an arbitrarily aligned address, widened to int
template <typename T, int W> __device__ __forceinline__ void dg_load(DG_GL const unsigned char *p, int *o) {
    constexpr int BYTES = W * (int)sizeof(T);
    unsigned d[(BYTES + 3) / 4];
    if (BYTES >= 16) {
#pragma unroll
        for (int k = 0; k < BYTES / 16; k++) { dg_uv4 t = *(DG_GL const dg_uv4 *)(p + 16 * k); d[4 * k] = t[0]; d[4 * k + 1] = t[1]; d[4 * k + 2] = t[2]; d[4 * k + 3] = t[3]; }
    } else if (BYTES == 8) { dg_uv2 t = *(DG_GL const dg_uv2 *)p; d[0] = t[0]; d[1] = t[1]; }
    else if (BYTES == 4) d[0] = *(DG_GL const dg_uv1 *)p;
    else d[0] = *(DG_GL const dg_uh1 *)p;
#pragma unroll
    for (int i = 0; i < W; i++) {
        if (sizeof(T) == 2) o[i] = (int)((d[i >> 1] >> (16 * (i & 1))) & 0xffffu);
        else o[i] = (int)((d[i >> 2] >> (8 * (i & 3))) & 0xffu);
    }
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
template <typename T, int W> __device__ __forceinline__ void dg_store(DG_GL unsigned char *p, const int *v) {
    constexpr int BYTES = W * (int)sizeof(T);
    unsigned d[(BYTES + 3) / 4];
#pragma unroll
    for (int k = 0; k < (BYTES + 3) / 4; k++) d[k] = 0;
#pragma unroll
    for (int i = 0; i < W; i++) {
        if (sizeof(T) == 2) d[i >> 1] |= (unsigned)v[i] << (16 * (i & 1));
        else d[i >> 2] |= (unsigned)v[i] << (8 * (i & 3));
    }
    if (BYTES >= 16) {
#pragma unroll
        for (int k = 0; k < BYTES / 16; k++) { dg_uv4 t = { d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3] }; *(DG_GL dg_uv4 *)(p + 16 * k) = t; }
    } else if (BYTES == 8) { dg_uv2 t = { d[0], d[1] }; *(DG_GL dg_uv2 *)p = t; }
    else if (BYTES == 4) *(DG_GL dg_uv1 *)p = d[0];
    else *(DG_GL dg_uh1 *)p = (unsigned short)d[0];
}

// SimpleResize.cpp:62-121, uint8_t form, at one output sample whose table values are at hand: rows r0 / r1 (byte offsets), column o,
// vertical weights wt / wb, horizontal weights wl / wr.  PTR: a generic or a global-address-space byte pointer.
template <typename PTR> __device__ __forceinline__ int fps_upsize_u8(PTR m, int r0, int r1, int o, int wt, int wb, int wl, int wr) {
    const int a = (unsigned char)((m[r0 + o] * wt + m[r1 + o] * wb + 8192) >> 14), b = (unsigned char)((m[r0 + o + 1] * wt + m[r1 + o + 1] * wb + 8192) >> 14);
    return (unsigned char)((a * wl + b * wr + 8192) >> 14);
}
// the same with the table lookups
__device__ __forceinline__ int bf_upsize(const unsigned char *m, int XP, const int *hOff, const int *hW, const int *vOff, const int *vW, int x, int y) {
    const int wb = vW[y], wr = hW[x], r0 = vOff[y] * XP;
    return fps_upsize_u8(m, r0, r0 + XP, hOff[x], 16384 - wb, wb, 16384 - wr, wr);
}

// Fakery.c:52-58,103-107,144-146 fgopIsUsable, the count part: this thread's share (stride 256) of the level-0 blocks whose SAD exceeds thscd1.
// Global-address-space loads, four in flight, so that a wave does not wait for each 16-byte record on its own.
__device__ __forceinline__ int fps_count_over(const unsigned char *blob, int nLvCount, int nBlk, long long thscd1) {
    DG_GL const unsigned char *v = dg_gl(mvx_level0(blob, nLvCount));
    int c = 0, i = threadIdx.x;
    for (; i + 768 < nBlk; i += 1024) {
        const long long s0 = *(DG_GL const long long *)(v + 16 * i + 8), s1 = *(DG_GL const long long *)(v + 16 * (i + 256) + 8);
        const long long s2 = *(DG_GL const long long *)(v + 16 * (i + 512) + 8), s3 = *(DG_GL const long long *)(v + 16 * (i + 768) + 8);
        c += (s0 > thscd1) + (s1 > thscd1) + (s2 > thscd1) + (s3 > thscd1);
    }
    for (; i < nBlk; i += 256) c += *(DG_GL const long long *)(v + 16 * i + 8) > thscd1 ? 1 : 0;
    return c;
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
