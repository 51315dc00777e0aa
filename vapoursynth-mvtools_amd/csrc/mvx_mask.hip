// mvx_mask.hip -- mv.Mask on gfx950: motion, SAD and occlusion masks from one vector clip (MVMask.c:75-211 frame, :227-346 creation,
// :66-72 mvmaskLength; MaskFun.cpp:85-166 ByteOccMask / MakeVectorOcclusionMaskTime / ByteNorm / MakeSADMaskTime; SimpleResize.cpp:27-121).
//
// The reference builds an nBlkX x nBlkY byte mask per frame (two for kind 5), upsizes it to the block-covered rectangle nWidthB x nHeightB
// of each plane, replicates column nWidthB - 1 to the right and then row nHeightB - 1 downwards, and copies U into V.  Here:
//   mask_usable_kernel : per (slice, job) -> the count of fgopIsUsable (Fakery.c:52-58,103-107,144-146); mk_usable decides from it
//   mask_small_kernel  : per (four blocks, job) -> the small masks, nBlkX * nBlkY bytes per job and plane, pitch nBlkX, no padding; kind 2
//                        scatter-maxes into an int plane (zeroed before) that mask_occ_finish_kernel turns into bytes
//   mask_planes_kernel : per 16 consecutive output bytes of a row -> one vector store, four rows per lane.  The upsizer's tables are built on the host
//                        for the whole plane with the coordinates clamped to the covered rectangle, which IS the edge replication
//                        (row-by-row vsh_bitblt semantics: every row below nHeightB - 1 equals it, after its right fill); V = U, the
//                        scene-change fill and kind 5's luma copy are cases of the same kernel.  One launch for the luma planes of all
//                        jobs, one for both chroma planes of all jobs.
// Deep objects (mvx_mask_create_deep, 9 to 16 bits; include/mvtools_amd.h has the semantics): the small masks stay bytes, kind 1 from the SAD >> (bits - 8)
// (mask_small_kernel<4, true>); mask_planes_kernel<CLS, 1> does a lane's work unchanged up to its 16 bytes and stores them as 16 samples of 16 bits.
// The instantiations <.., false> and <.., 0> are the 8-bit kernels, instruction for instruction what they were before the deep forms existed.
// pow: the device's double-precision pow where the exponent is not exactly 1; at exponent 1 the base itself (mvx_degrain.hip's SAD mask
// does the same), so kinds 1 and 2 at the default gamma 1 (and kind 0 at gamma 2) are exact whatever the two pow implementations do in the
// last place.  Kind 0 at gamma 1 is pow(x, 0.5): see DESIGN.md 4.9 for what that means for a byte.
#include <math.h>
#include "mvx_fps_shared.h"

struct MKParams {
    int kind, pel, isb, time256, ysc;
    int nBlkX, nBlkY, nBlk, nLvCount, stepX, stepY;
    int stride;                           // cells per small-mask plane: nBlk rounded up to 16
    long long thscd1; int thscd2;
    float fNorm, fNorm2, fHalfGamma;      // fMaskNormFactor, fMaskNormFactor2, fHalfGamma (MVMask.c:304-307): floats, as in the reference
    double gamma, halfGamma;              // (double)fGamma, (double)fHalfGamma
    double sadFactor;                     // 4.0 * fMaskNormFactor / (nBlkSizeX * nBlkSizeY), MVMask.c:143
    double occDivider;                    // 1.0 / fMaskNormFactor, MVMask.c:145
    int W[2], H[2], segs[2];              // luma / chroma plane size, 16-byte segments per row
    long long dstPitch[3], clipPitch;
    const unsigned *hTab[2], *vTab[2];    // per output column / row: small-mask offset << 16 | weight of the second cell (0..16384)
    int shift;                            // deep objects: the output depth - 8 (0..8); 0 otherwise.  Last, so that every earlier field keeps its offset
};
struct MKJob { const unsigned char *blob, *clip; unsigned char *dst[3]; };

// Fakery.c:52-58,103-107,144-146 fgopIsUsable, the count part.  One block per job reads 16 bytes per vector block through 256 lanes and is
// bound by latency (2 MB per job at 1080p), so a job's blocks are counted by MK_SLICES workgroups, each over one contiguous share, into
// over[job][MK_SLICES]; mk_usable sums them and decides.  A NULL blob counts nothing.
#define MK_SLICES 16
__global__ __launch_bounds__(256) void mask_usable_kernel(const MKParams *Pp, const MKJob *jobs, int *over) {
    const MKParams &P = *Pp;
    const int f = blockIdx.y, s = blockIdx.x;
    const unsigned char *blob = jobs[f].blob;
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    if (blob) {
        const int share = (P.nBlk + MK_SLICES - 1) / MK_SLICES, first = min(s * share, P.nBlk);
        const int c = fps_count_over(blob, P.nLvCount, first, min(share, P.nBlk - first), P.thscd1);
        if (c) atomicAdd(&cnt, c);
    }
    __syncthreads();
    if (threadIdx.x == 0) over[f * MK_SLICES + s] = cnt;
}
// the decision: the blob is there, valid, and no more than thscd2 of its blocks exceed thscd1
__device__ __forceinline__ bool mk_usable(const MKParams &P, const unsigned char *blob, const int *over) {
    if (!blob || ((const int *)blob)[1] != 1) return false;
    int c = 0;
#pragma unroll
    for (int k = 0; k < MK_SLICES; k++) c += over[k];
    return !(c > P.thscd2);
}

// pow(b, e) of the reference, without the call where e is exactly 1
__device__ __forceinline__ double mk_pow(double b, double e) { return e == 1.0 ? b : pow(b, e); }
// (uint8_t)((l > 255) ? 255 : l), MVMask.c:71 / MaskFun.cpp:138
__device__ __forceinline__ unsigned char mk_cut(double l) { return (unsigned char)((l > 255) ? 255 : l); }
// MVMask.c:148-156: float arithmetic, left to right, unfused
__device__ __forceinline__ unsigned char mk_component(int v, float f) { return (unsigned char)max(0, min(255, (int)(v * f * 100 + 128))); }

// small[job][2][stride] bytes (the second plane: kind 5's V); occ[job][stride] ints, kind 2 only
// NB = 4: one lane computes four consecutive blocks and stores their bytes as one dword (a byte store per lane costs as much as a dword
// store); the four 16-byte vector records are loaded together.  NB = 1 is kind 2's form: it stores nothing here, and four scatters per lane
// only lengthen the chain of atomics (measured: 0.152 -> 0.179 ms per 64 frames).  A plane holds P.stride bytes, nBlk rounded up to 16, so
// every job's planes are aligned.
// SH: the deep form of kind 1, MaskFun.cpp:162 with bitsPerSample the clip argument's: the int64 SAD >> P.shift (arithmetic) before it becomes a double
template <int NB, bool SH>
__global__ __launch_bounds__(256) void mask_small_kernel(const MKParams *Pp, const MKJob *jobs, const int *over, unsigned char *small, int *occ) {
    const MKParams &P = *Pp;
    const int f = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * NB;
    if (i0 >= P.nBlk || !mk_usable(P, jobs[f].blob, over + f * MK_SLICES)) return;
    const GVecD *vec = mvx_level0(jobs[f].blob, P.nLvCount);
    unsigned char *m = small + (size_t)f * 2 * P.stride;
    const int nBlkX = P.nBlkX, nBlkY = P.nBlkY;
    int vx[NB], vy[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) { const int i = min(i0 + k, P.nBlk - 1); vx[k] = vec[i].x; vy[k] = vec[i].y; }
    unsigned b0 = 0, b1 = 0;
#pragma unroll
    for (int k = 0; k < NB; k++) {
        const int i = i0 + k;
        if (i >= P.nBlk) break;
        const int by = i / nBlkX, bx = i - by * nBlkX;
        unsigned c = 0;
        if (P.kind == 0) { // mvmaskLength: the integer sum in int as written (wrapping made explicit)
            const int n2 = (int)((unsigned)vx[k] * (unsigned)vx[k] + (unsigned)vy[k] * (unsigned)vy[k]);
            const double norme = (double)n2 / (P.pel * P.pel);
            c = mk_cut(255 * mk_pow(norme * P.fNorm2, P.halfGamma));
        } else if (P.kind == 1) { // MakeSADMaskTime; the SAD shift is that of the 8-bit mask clip: none
            const int tX = (256 - P.time256) * 16 / (P.stepX * P.pel), tY = (256 - P.time256) * 16 / (P.stepY * P.pel);
            int bxi = bx - vx[k] * tX / 4096, byi = by - vy[k] * tY / 4096;
            if (bxi < 0 || bxi >= nBlkX || byi < 0 || byi >= nBlkY) { bxi = bx; byi = by; }
            const long long sad = SH ? vec[bxi + byi * nBlkX].sad >> P.shift : vec[bxi + byi * nBlkX].sad;
            c = mk_cut(255 * mk_pow(sad * P.sadFactor, P.gamma));
        } else if (P.kind == 2) {
            fps_occlusion_block(vec, i, bx, by, nBlkX, nBlkY, P.isb, P.time256, P.stepX, P.stepY, P.pel, P.occDivider, occ + (size_t)f * P.stride, nBlkX, P.gamma);
        } else if (P.kind == 4) {
            c = mk_component(vy[k], P.fNorm);
        } else { // 3, and 5's U
            c = mk_component(vx[k], P.fNorm);
            if (P.kind == 5) b1 |= (unsigned)mk_component(vy[k], P.fNorm) << (8 * k);
        }
        b0 |= c << (8 * k);
    }
    if (NB == 1 || P.kind == 2) return;
    *(unsigned *)(m + i0) = b0;
    if (P.kind == 5) *(unsigned *)(m + P.stride + i0) = b1;
}
// kind 2: the scatter-maxed ints as bytes, four per lane
__global__ __launch_bounds__(256) void mask_occ_finish_kernel(const MKParams *Pp, const MKJob *jobs, const int *over, const int *occ, unsigned char *small) {
    const MKParams &P = *Pp;
    const int f = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= P.nBlk || !mk_usable(P, jobs[f].blob, over + f * MK_SLICES)) return;
    const dg_iv4 t = *(const dg_iv4 *)(occ + (size_t)f * P.stride + i0);
    *(unsigned *)(small + (size_t)f * 2 * P.stride + i0) = (unsigned)t[0] | (unsigned)t[1] << 8 | (unsigned)t[2] << 16 | (unsigned)t[3] << 24;
}

// n (1..16) bytes, lo the first eight and hi the rest, to the 16-byte aligned address d: one vector store, or for a row's tail the pieces
// 8 / 4 / 2 / 1 of n, each aligned
__device__ __forceinline__ void mk_store(DG_GL unsigned char *d, unsigned long long lo, unsigned long long hi, int n) {
    if (n == 16) { const dg_iv4 t = { (int)lo, (int)(lo >> 32), (int)hi, (int)(hi >> 32) }; *(DG_GL dg_iv4 *)d = t; return; }
    unsigned long long r = lo; // the bytes not yet stored
    int o = 0;
    if (n & 8) { const dg_iv2 t = { (int)lo, (int)(lo >> 32) }; *(DG_GL dg_iv2 *)d = t; r = hi; o = 8; }
    if (n & 4) { *(DG_GL unsigned *)(d + o) = (unsigned)r; r >>= 32; o += 4; }
    if (n & 2) { *(DG_GL unsigned short *)(d + o) = (unsigned short)r; r >>= 16; o += 2; }
    if (n & 1) d[o] = (unsigned char)r;
}

// The deep forms.  mk_widen: four bytes of w as four 16-bit samples E(m) in two dwords, E(m) = m << shl | m >> shr on every 16-bit lane.  A weight
// (kinds 0-2) replicates its bits, shr = 8 - shl: 0 stays 0 and 255 becomes the peak; an offset (kinds 3-5) passes shr = 8, m >> 8 = 0: 128 becomes half
// the range.  m << shl stays inside its lane (255 << 8 < 65536); m >> shr lets bits of the upper lane into the lower one, which the mask removes.
__device__ __forceinline__ void mk_widen(unsigned w, int shl, int shr, unsigned &a, unsigned &b) {
    const unsigned p = __builtin_amdgcn_perm(0u, w, 0x0c010c00u), q = __builtin_amdgcn_perm(0u, w, 0x0c030c02u);
    a = (p << shl) | ((p >> shr) & 0x00ff00ffu);
    b = (q << shl) | ((q >> shr) & 0x00ff00ffu);
}
// n (1..16) 16-bit samples, four per q, to the 16-byte aligned address d: two adjacent vector stores, or for a row's tail the pieces 8 / 4 / 2 / 1 of
// n, each aligned
__device__ __forceinline__ void mk_store16(DG_GL unsigned char *d, unsigned long long q0, unsigned long long q1, unsigned long long q2, unsigned long long q3, int n) {
    if (n == 16) {
        const dg_iv4 t = { (int)q0, (int)(q0 >> 32), (int)q1, (int)(q1 >> 32) }, u = { (int)q2, (int)(q2 >> 32), (int)q3, (int)(q3 >> 32) };
        *(DG_GL dg_iv4 *)d = t; *(DG_GL dg_iv4 *)(d + 16) = u;
        return;
    }
    unsigned long long a = q0, b = q1; // the samples not yet stored: the next four, and the four after them
    int o = 0;
    if (n & 8) { const dg_iv4 t = { (int)q0, (int)(q0 >> 32), (int)q1, (int)(q1 >> 32) }; *(DG_GL dg_iv4 *)d = t; a = q2; b = q3; o = 16; }
    if (n & 4) { const dg_iv2 t = { (int)a, (int)(a >> 32) }; *(DG_GL dg_iv2 *)(d + o) = t; a = b; o += 8; }
    if (n & 2) { *(DG_GL unsigned *)(d + o) = (unsigned)a; a >>= 32; o += 4; }
    if (n & 1) *(DG_GL unsigned short *)(d + o) = (unsigned short)a;
}
// the 16 bytes w of one segment of a row, widened to n samples at d
__device__ __forceinline__ void mk_store_wide(DG_GL unsigned char *d, const unsigned *w, int n, int shl, int shr) {
    unsigned e[8];
#pragma unroll
    for (int k = 0; k < 4; k++) mk_widen(w[k], shl, shr, e[2 * k], e[2 * k + 1]);
    mk_store16(d, e[0] | (unsigned long long)e[1] << 32, e[2] | (unsigned long long)e[3] << 32, e[4] | (unsigned long long)e[5] << 32, e[6] | (unsigned long long)e[7] << 32, n);
}

// 16 bytes from any address as four dwords: aligned dword loads (gfx950 serves vector loads at odd addresses several times slower) and a
// byte rotation.  Reads up to 20 bytes from the address rounded down to a dword: the small masks are allocated with that slack.
__device__ __forceinline__ void mk_load16(DG_GL const unsigned char *p, unsigned *o) {
    const unsigned long long a = (unsigned long long)p;
    DG_GL const unsigned char *q = (DG_GL const unsigned char *)(a & ~3ull);
    const unsigned sh = (unsigned)a & 3u;
    const dg_iv4 t = *(DG_GL const dg_iv4 *)q;
    const unsigned t4 = *(DG_GL const unsigned *)(q + 16);
    o[0] = __builtin_amdgcn_alignbyte((unsigned)t[1], (unsigned)t[0], sh); o[1] = __builtin_amdgcn_alignbyte((unsigned)t[2], (unsigned)t[1], sh);
    o[2] = __builtin_amdgcn_alignbyte((unsigned)t[3], (unsigned)t[2], sh); o[3] = __builtin_amdgcn_alignbyte(t4, (unsigned)t[3], sh);
}
// the same for 8 bytes (reads up to 12 from the rounded address)
__device__ __forceinline__ void mk_load8(DG_GL const unsigned char *p, unsigned *o) {
    const unsigned long long a = (unsigned long long)p;
    DG_GL const unsigned char *q = (DG_GL const unsigned char *)(a & ~3ull);
    const unsigned sh = (unsigned)a & 3u;
    const dg_iv2 t = *(DG_GL const dg_iv2 *)q;
    const unsigned t2 = *(DG_GL const unsigned *)(q + 8);
    o[0] = __builtin_amdgcn_alignbyte((unsigned)t[1], (unsigned)t[0], sh); o[1] = __builtin_amdgcn_alignbyte(t2, (unsigned)t[1], sh);
}
// lo(a) * lo(w) + hi(a) * hi(w) + 8192 on 16-bit halves: one step of the upsizer before its shift
typedef unsigned short mk_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned mk_dot(unsigned a, unsigned w) {
    mk_us2 x, y;
    __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&y, &w, 4);
    return __builtin_amdgcn_udot2(x, y, 8192u, false);
}

// SimpleResize.cpp:82-87, the vertical pass over 4 * N cells: t the upper row's bytes, u the lower row's, wv = wt | wb << 16
template <int N> __device__ __forceinline__ void mk_vertical(const unsigned *t, const unsigned *u, unsigned wv, unsigned *v) {
#pragma unroll
    for (int k = 0; k < N; k++) {
        v[k] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) // low half: cell j of the upper row, high half: of the lower row
            v[k] |= (mk_dot(__builtin_amdgcn_perm(u[k], t[k], 0x0c000c00u + j + ((4 + j) << 16)), wv) >> 14) << (8 * j);
    }
}
// SimpleResize.cpp:89-95, the horizontal pass at one sample: cells c and c + 1 (c <= 6) of the 8-cell window lo / hi, wr the weight of the second
__device__ __forceinline__ unsigned mk_sample(unsigned lo, unsigned hi, int c, unsigned wr) {
    const unsigned pair = __builtin_amdgcn_perm(hi, lo, 0x0c010c00u + (unsigned)c * 0x00010001u);
    return mk_dot(pair, wr * 0xffffu + 16384u) >> 14; // the weights (16384 - wr) | wr << 16
}

// CLS 0: the luma planes of all jobs (blockIdx.y = job); CLS 1: both chroma planes (blockIdx.y = job * 2 + plane - 1).
// A lane produces the same 16-byte segment of MK_ROWS consecutive rows.  With one row per lane the kernel is bound by latency, not by the
// stores: a wave lives for four dependent memory round trips (job, usable, tables, cells) and moves 1 KB.  The rows of a lane share the
// horizontal table entries and the usable test, and their cell loads are all in flight together.
// DEEP: the form for 16-bit samples.  A lane's work is the same up to the 16 bytes it would store; they leave as 16 samples E(m), two adjacent
// 16-byte stores per row (a wave: 2 KB contiguous), the fill as E(ysc), and kind 5's luma is copied two bytes a sample.
#define MK_ROWS 4
template <int CLS, int DEEP>
__global__ __launch_bounds__(256) void mask_planes_kernel(const MKParams *Pp, const MKJob *jobs, const int *over, const unsigned char *small) {
    const MKParams &P = *Pp;
    const int f = CLS ? blockIdx.y >> 1 : blockIdx.y, pl = CLS ? 1 + (blockIdx.y & 1) : 0;
    const int segs = P.segs[CLS], H = P.H[CLS];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int yg = idx / segs, s = idx - yg * segs, y0 = yg * MK_ROWS;
    if (y0 >= H) return;
    const MKJob &J = jobs[f];
    const int x0 = 16 * s, n = min(16, P.W[CLS] - x0);
    const long long pitch = P.dstPitch[pl];
    DG_GL unsigned char *d = dg_glw(J.dst[pl]) + (long long)y0 * pitch + (DEEP ? 2 * x0 : x0);
    const int shl = DEEP ? P.shift : 0, shr = DEEP && P.kind <= 2 ? 8 - shl : 8; // mk_widen: a weight for kinds 0-2, an offset for kinds 3-5
    if (DEEP && CLS == 0 && P.kind == 5) { // the clip's luma at its own depth
        DG_GL const unsigned char *c = dg_gl(J.clip) + (long long)y0 * P.clipPitch + 2 * x0;
        unsigned w[MK_ROWS][8];
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++) {
#pragma unroll
            for (int k = 0; k < 8; k++) w[r][k] = 0;
            if (y0 + r >= H) continue;
            DG_GL const unsigned char *cr = c + r * P.clipPitch;
            if (n == 16) {
                const dg_uv4 t = *(DG_GL const dg_uv4 *)cr, u = *(DG_GL const dg_uv4 *)(cr + 16);
#pragma unroll
                for (int k = 0; k < 4; k++) { w[r][k] = t[k]; w[r][4 + k] = u[k]; }
            } else {
#pragma unroll
                for (int i = 0; i < 15; i++) if (i < n) w[r][i >> 1] |= (unsigned)*(DG_GL const dg_uh1 *)(cr + 2 * i) << (16 * (i & 1));
            }
        }
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++)
            if (y0 + r < H) mk_store16(d + r * pitch, w[r][0] | (unsigned long long)w[r][1] << 32, w[r][2] | (unsigned long long)w[r][3] << 32,
                                       w[r][4] | (unsigned long long)w[r][5] << 32, w[r][6] | (unsigned long long)w[r][7] << 32, n);
        return;
    }
    if (!DEEP && CLS == 0 && P.kind == 5) { // MVMask.c:160-161,194-195: the clip's luma, usable or not
        DG_GL const unsigned char *c = dg_gl(J.clip) + (long long)y0 * P.clipPitch + x0;
        unsigned w[MK_ROWS][4];
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++) {
            w[r][0] = w[r][1] = w[r][2] = w[r][3] = 0;
            if (y0 + r >= H) continue;
            DG_GL const unsigned char *cr = c + r * P.clipPitch;
            if (n == 16) { const dg_uv4 t = *(DG_GL const dg_uv4 *)cr; w[r][0] = t[0]; w[r][1] = t[1]; w[r][2] = t[2]; w[r][3] = t[3]; }
            else {
#pragma unroll
                for (int i = 0; i < 15; i++) if (i < n) w[r][i >> 2] |= (unsigned)cr[i] << (8 * (i & 3));
            }
        }
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++)
            if (y0 + r < H) mk_store(d + r * pitch, w[r][0] | (unsigned long long)w[r][1] << 32, w[r][2] | (unsigned long long)w[r][3] << 32, n);
        return;
    }
    if (!mk_usable(P, J.blob, over + f * MK_SLICES)) { // MVMask.c:197-200
        const unsigned long long fill = (unsigned)P.ysc * 0x0101010101010101ull;
        if (DEEP) { // E(ysc) by the plane's rule
            const unsigned long long fill16 = (unsigned long long)((unsigned)P.ysc << shl | (unsigned)P.ysc >> shr) * 0x0001000100010001ull;
#pragma unroll
            for (int r = 0; r < MK_ROWS; r++)
                if (y0 + r < H) mk_store16(d + r * pitch, fill16, fill16, fill16, fill16, n);
            return;
        }
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++)
            if (y0 + r < H) mk_store(d + r * pitch, fill, fill, n);
        return;
    }
    DG_GL const unsigned char *m = dg_gl(small) + ((size_t)f * 2 + (P.kind == 5 && pl == 2 ? 1 : 0)) * P.stride;
    unsigned e[16];
    DG_GL const unsigned char *ht = (DG_GL const unsigned char *)(unsigned long long)(P.hTab[CLS] + x0); // the table is padded to whole segments
#pragma unroll
    for (int k = 0; k < 4; k++) { const dg_iv4 t = *(DG_GL const dg_iv4 *)(ht + 16 * k); e[4 * k] = t[0]; e[4 * k + 1] = t[1]; e[4 * k + 2] = t[2]; e[4 * k + 3] = t[3]; }
    // the rows' vertical entries (the table is padded to whole groups of rows): the pair of small-mask rows and its weights, once per segment
    const dg_iv4 ve = *(DG_GL const dg_iv4 *)(unsigned long long)(P.vTab[CLS] + y0);
    DG_GL const unsigned char *m0[MK_ROWS];
    unsigned wv[MK_ROWS];
#pragma unroll
    for (int r = 0; r < MK_ROWS; r++) {
        const unsigned v = (unsigned)ve[r], wb = v & 0xffffu;
        m0[r] = m + (int)(v >> 16) * P.nBlkX;
        wv[r] = (16384u - wb) | wb << 16;
    }
    // The usual cases (two or more samples per cell): the cells from oF on of both small-mask rows in two loads each, the vertical pass over
    // all of them as packed dot products, then every sample picks its pair of neighbours out of an 8-cell window.  Same integers as the
    // general form below: (t * wt + b * wb + 8192) >> 14 is below 256, so the reference's byte cast changes nothing.
    const int oF = (int)(e[0] >> 16), o7 = (int)(e[7] >> 16), o8 = (int)(e[8] >> 16), oL = (int)(e[15] >> 16);
    if (oL - oF <= 6) { // the segment spans at most 8 cells (nearly three samples per cell or more): one window
        unsigned t[MK_ROWS][2], u[MK_ROWS][2];
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++) { mk_load8(m0[r] + oF, t[r]); mk_load8(m0[r] + P.nBlkX + oF, u[r]); }
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++) {
            unsigned v[2], w[4] = { 0, 0, 0, 0 };
            mk_vertical<2>(t[r], u[r], wv[r], v);
#pragma unroll
            for (int i = 0; i < 16; i++) w[i >> 2] |= mk_sample(v[0], v[1], (int)(e[i] >> 16) - oF, e[i] & 0xffffu) << (8 * (i & 3));
            if (DEEP) { if (y0 + r < H) mk_store_wide(d + r * pitch, w, n, shl, shr); }
            else if (y0 + r < H) mk_store(d + r * pitch, w[0] | (unsigned long long)w[1] << 32, w[2] | (unsigned long long)w[3] << 32, n);
        }
    } else if (o7 - oF <= 6 && oL - o8 <= 6 && o8 - oF <= 8) { // at most 16 cells, each half at most 8: a window per half
        unsigned t[MK_ROWS][4], u[MK_ROWS][4];
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++) { mk_load16(m0[r] + oF, t[r]); mk_load16(m0[r] + P.nBlkX + oF, u[r]); }
        const int k8 = o8 - oF, q = k8 >> 2;
#pragma unroll
        for (int r = 0; r < MK_ROWS; r++) {
            unsigned v[4], w[4] = { 0, 0, 0, 0 };
            mk_vertical<4>(t[r], u[r], wv[r], v);
            const unsigned A = q == 0 ? v[0] : q == 1 ? v[1] : v[2], B = q == 0 ? v[1] : q == 1 ? v[2] : v[3], Cc = q == 0 ? v[2] : q == 1 ? v[3] : 0u;
            const unsigned x0w = __builtin_amdgcn_alignbyte(B, A, k8 & 3), x1w = __builtin_amdgcn_alignbyte(Cc, B, k8 & 3);
#pragma unroll
            for (int i = 0; i < 8; i++) w[i >> 2] |= mk_sample(v[0], v[1], (int)(e[i] >> 16) - oF, e[i] & 0xffffu) << (8 * (i & 3));
#pragma unroll
            for (int i = 8; i < 16; i++) w[i >> 2] |= mk_sample(x0w, x1w, (int)(e[i] >> 16) - o8, e[i] & 0xffffu) << (8 * (i & 3));
            if (DEEP) { if (y0 + r < H) mk_store_wide(d + r * pitch, w, n, shl, shr); }
            else if (y0 + r < H) mk_store(d + r * pitch, w[0] | (unsigned long long)w[1] << 32, w[2] | (unsigned long long)w[3] << 32, n);
        }
    } else {
        // SimpleResize.cpp:62-121 at any geometry: the vertical pass rounded to a byte per small-mask column, then the horizontal pass; a
        // column's vertical result is kept while the offset stays and handed on when it advances by one
        for (int r = 0; r < MK_ROWS && y0 + r < H; r++) {
            DG_GL const unsigned char *ma = m0[r], *mb = ma + P.nBlkX;
            const int wt = (int)(wv[r] & 0xffffu), wb = (int)(wv[r] >> 16);
            unsigned w[4] = { 0, 0, 0, 0 };
            int cur = -2, a = 0, b = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int o = (int)(e[i] >> 16), wr = (int)(e[i] & 0xffffu);
                if (o != cur) {
                    a = o == cur + 1 ? b : (int)(unsigned char)((ma[o] * wt + mb[o] * wb + 8192) >> 14);
                    b = (int)(unsigned char)((ma[o + 1] * wt + mb[o + 1] * wb + 8192) >> 14);
                    cur = o;
                }
                w[i >> 2] |= (unsigned)(unsigned char)((a * (16384 - wr) + b * wr + 8192) >> 14) << (8 * (i & 3));
            }
            if (DEEP) mk_store_wide(d + r * pitch, w, n, shl, shr);
            else mk_store(d + r * pitch, w[0] | (unsigned long long)w[1] << 32, w[2] | (unsigned long long)w[3] << 32, n);
        }
    }
}


// ------------------------------------------------------------------------------------------------ host object

struct mvx_mask {
    CallGuard guard;
    MKParams P;
    mvx_mask_info info;
    int bits;                            // of the output samples: 8, or a deep object's 9..16 (two bytes a sample)
    std::vector<unsigned> tables;       // hTab luma, vTab luma, hTab chroma, vTab chroma
    size_t tabOff[4];
    DevBuf<MKParams> dP;
    DevBuf<unsigned> dTables;
    DevBuf<MKJob> dJobs;                 // the per-job buffers hold exactly the largest call's jobs
    DevBuf<int> dOver, dOcc;
    DevBuf<unsigned char> dSmall;
};

// SimpleResize.cpp:27-57 InitTables from `in` cells to `covered` samples, laid out for all `size` samples of the plane (and on to `padded`
// entries): a sample beyond the covered rectangle takes the entry of the last covered one -- MVMask.c:164-169,180-189
static void mask_table(unsigned *t, int padded, int size, int covered, int in) {
    std::vector<int> o(covered), w(covered);
    bf_tables(o.data(), w.data(), covered, in);
    for (int i = 0; i < padded; i++) {
        const int k = std::min(std::min(i, size - 1), covered - 1);
        t[i] = ((unsigned)o[k] << 16) | (unsigned)w[k];
    }
}

// MVMask.c:227-346 mvmaskCreate.  deep: the format check of mvx_mask_create_deep, and an output of the clip's depth
static int mask_create(const mvx_mask_args *a, const mvx_analysis_data *ad, const mvx_mask_clip *clip, const ptrdiff_t clip_pitch[3],
        const ptrdiff_t dst_pitch[3], mvx_mask **out, char *err, bool deep) {
    MVX_CREATE_BEGIN(out);
    const float ml = (float)a->ml, fGamma = (float)a->gamma;   // float arguments (MVMask.c:235-241)
    const int kind = a->kind == MVX_UNSET ? 0 : a->kind;
    const double time = a->time;
    const int ysc = a->ysc == MVX_UNSET ? 0 : a->ysc;
    int64_t thscd1; int32_t thscd2;
    if (fGamma < 0.0f) MVX_FAIL("Mask: gamma must not be negative.");
    if (kind < 0 || kind > 5) MVX_FAIL("Mask: kind must 0, 1, 2, 3, 4, or 5.");
    if (time < 0.0 || time > 100.0) MVX_FAIL("Mask: time must be between 0.0 and 100.0 (inclusive).");
    if (ysc < 0 || ysc > 255) MVX_FAIL("Mask: ysc must be between 0 and 255 (inclusive).");
    if (int rc = mvx_resolve_thscd("Mask", a->thscd1, a->thscd2, ad, &thscd1, &thscd2, err)) return rc;
    const bool subOk = clip->subsampling_w >= 0 && clip->subsampling_w <= 1 && clip->subsampling_h >= 0 && clip->subsampling_h <= 1;
    if (deep && (clip->bits < 8 || clip->bits > 16 || !subOk))
        MVX_FAIL("Mask: input clip must be Gray or YUV (4:2:0, 4:2:2, 4:4:0, 4:4:4) of 8 to 16 bits, with constant dimensions.");
    if (!deep && (clip->bits > 8 || !subOk))
        MVX_FAIL("Mask: input clip must be GRAY8, YUV420P8, YUV422P8, YUV440P8, or YUV444P8, with constant dimensions.");
    // the library's own checks (divergences 1 and 2 of mvtools_amd.h)
    if (ad->nBlkX < 2 || ad->nBlkY < 2) MVX_FAIL("Mask: the frame must be at least two blocks wide and two blocks high.");
    const int xr = clip->gray ? 1 : 1 << clip->subsampling_w, yr = clip->gray ? 1 : 1 << clip->subsampling_h;
    if (clip->width != ad->nWidth || clip->height != ad->nHeight || xr != ad->xRatioUV || yr != ad->yRatioUV)
        MVX_FAIL("Mask: the clip's size and chroma subsampling must be those of the vector clip.");
    if (dst_pitch[0] % 16 || dst_pitch[1] % 16 || dst_pitch[1] != dst_pitch[2]) MVX_FAIL("Mask: dst pitches must be multiples of 16 bytes, U and V alike.");

    mvx_mask *h = new mvx_mask();
    MKParams &P = h->P;
    memset(&P, 0, sizeof(P));
    P.kind = kind; P.pel = ad->nPel; P.isb = ad->isBackward; P.ysc = ysc;
    P.time256 = (int)(time * 256 / 100);                       // MVMask.c:334, in double
    P.nBlkX = ad->nBlkX; P.nBlkY = ad->nBlkY; P.nBlk = ad->nBlkX * ad->nBlkY; P.nLvCount = ad->nLvCount;
    P.stride = (P.nBlk + 15) / 16 * 16;
    P.stepX = ad->nBlkSizeX - ad->nOverlapX; P.stepY = ad->nBlkSizeY - ad->nOverlapY;
    P.thscd1 = thscd1; P.thscd2 = thscd2;
    P.fNorm = 1.0f / ml;                                       // MVMask.c:304-307
    P.fNorm2 = P.fNorm * P.fNorm;
    P.fHalfGamma = fGamma * 0.5f;
    P.gamma = fGamma; P.halfGamma = P.fHalfGamma;
    P.sadFactor = 4.0 * P.fNorm / (ad->nBlkSizeX * ad->nBlkSizeY);
    P.occDivider = 1.0 / P.fNorm;
    const int nWidthB = ad->nBlkX * P.stepX + ad->nOverlapX, nHeightB = ad->nBlkY * P.stepY + ad->nOverlapY; // MVMask.c:309-315
    const int covW[2] = { nWidthB, nWidthB / ad->xRatioUV }, covH[2] = { nHeightB, nHeightB / ad->yRatioUV };
    P.W[0] = ad->nWidth; P.H[0] = ad->nHeight; P.W[1] = ad->nWidth / ad->xRatioUV; P.H[1] = ad->nHeight / ad->yRatioUV;
    size_t total = 0;
    for (int c = 0; c < 2; c++) {
        P.segs[c] = (P.W[c] + 15) / 16;
        h->tabOff[2 * c] = total; total += (size_t)P.segs[c] * 16;
        h->tabOff[2 * c + 1] = total; total += (size_t)(P.H[c] + 3) / 4 * 4;
    }
    h->tables.resize(total);
    for (int c = 0; c < 2; c++) {
        mask_table(h->tables.data() + h->tabOff[2 * c], P.segs[c] * 16, P.W[c], covW[c], ad->nBlkX);
        mask_table(h->tables.data() + h->tabOff[2 * c + 1], (P.H[c] + 3) / 4 * 4, P.H[c], covH[c], ad->nBlkY);
    }
    for (int p = 0; p < 3; p++) P.dstPitch[p] = dst_pitch[p];
    P.clipPitch = clip_pitch ? clip_pitch[0] : 0;
    mvx_mask_info &I = h->info;
    memset(&I, 0, sizeof(I));
    I.width = ad->nWidth; I.height = ad->nHeight; I.num_planes = 3;
    I.subsampling_w = clip->gray ? 0 : clip->subsampling_w; I.subsampling_h = clip->gray ? 0 : clip->subsampling_h;
    for (int p = 0; p < 3; p++) { I.plane_width[p] = P.W[p ? 1 : 0]; I.plane_height[p] = P.H[p ? 1 : 0]; }
    I.time256 = P.time256; I.fMaskNormFactor = P.fNorm; I.fMaskNormFactor2 = P.fNorm2; I.fHalfGamma = P.fHalfGamma;
    h->bits = deep ? clip->bits : 8;
    P.shift = h->bits - 8;
    *out = h;
    return MVX_OK;
}
extern "C" __attribute__((visibility("default"))) int mvx_mask_create(const mvx_mask_args *a, const mvx_analysis_data *ad, const mvx_mask_clip *clip,
        const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_mask **out, char *err) {
    return mask_create(a, ad, clip, clip_pitch, dst_pitch, out, err, false);
}
extern "C" __attribute__((visibility("default"))) int mvx_mask_create_deep(const mvx_mask_args *a, const mvx_analysis_data *ad, const mvx_mask_clip *clip,
        const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_mask **out, char *err) {
    return mask_create(a, ad, clip, clip_pitch, dst_pitch, out, err, true);
}
extern "C" __attribute__((visibility("default"))) int mvx_mask_out_bits(const mvx_mask *h) { return h->bits; }
extern "C" __attribute__((visibility("default"))) void mvx_mask_destroy(mvx_mask *h) { delete h; }
extern "C" __attribute__((visibility("default"))) void mvx_mask_get_info(const mvx_mask *h, mvx_mask_info *info) { *info = h->info; }

// MVMask.c:75-211 mvmaskGetFrame
extern "C" __attribute__((visibility("default"))) int mvx_mask_frames(mvx_mask *h, int nframes, const mvx_mask_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    if (nframes > 32767) { mvx_set_error("mvx_mask_frames: at most 32767 jobs per call"); return MVX_E_ARG; }
    hipStream_t st = (hipStream_t)stream;
    CallGuard::Scope scope(h->guard, st);
    MKParams &P = h->P;
    std::vector<MKJob> hj(nframes);
    for (int f = 0; f < nframes; f++) {
        const mvx_mask_job &s = jobs[f];
        MKJob &j = hj[f];
        j.blob = (const unsigned char *)s.blob; j.clip = (const unsigned char *)s.clip_luma;
        for (int p = 0; p < 3; p++) {
            j.dst[p] = (unsigned char *)s.dst[p];
            if (!j.dst[p] || ((uintptr_t)j.dst[p] & 15)) { mvx_set_error("mvx_mask_frames: three dst planes are required, 16-byte aligned"); return MVX_E_ARG; }
        }
        if (P.kind == 5 && !j.clip) { mvx_set_error("mvx_mask_frames: kind 5 needs clip_luma"); return MVX_E_ARG; }
    }
    if (!h->dP.p) {
        HIP_CHECK(h->dTables.reserve(h->tables.size()));
        HIP_CHECK(hipMemcpy(h->dTables.p, h->tables.data(), sizeof(unsigned) * h->tables.size(), hipMemcpyHostToDevice));
        for (int c = 0; c < 2; c++) { P.hTab[c] = h->dTables.p + h->tabOff[2 * c]; P.vTab[c] = h->dTables.p + h->tabOff[2 * c + 1]; }
        HIP_CHECK(h->dP.reserve(1));
        if (hipMemcpy(h->dP.p, &P, sizeof(MKParams), hipMemcpyHostToDevice) != hipSuccess) { h->dP.release(); mvx_set_error("mvx_mask_frames: parameter upload failed"); return MVX_E_DEVICE; }
    }
    const size_t n = (size_t)nframes;
    HIP_CHECK(h->dJobs.reserve(n));
    HIP_CHECK(h->dOver.reserve(n * MK_SLICES));
    HIP_CHECK(h->dSmall.reserve(n * 2 * (size_t)P.stride + 32)); // + the slack mk_load16 may read
    if (P.kind == 2) HIP_CHECK(h->dOcc.reserve(n * (size_t)P.stride));
    HIP_CHECK(hipMemcpyAsync(h->dJobs.p, hj.data(), sizeof(MKJob) * nframes, hipMemcpyHostToDevice, st));
    const dim3 perBlock((unsigned)(((P.nBlk + 3) / 4 + 255) / 256), (unsigned)nframes); // four blocks per lane
    hipLaunchKernelGGL(mask_usable_kernel, dim3(MK_SLICES, (unsigned)nframes), dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p);
    if (P.kind == 2) HIP_CHECK(hipMemsetAsync(h->dOcc.p, 0, n * P.stride * sizeof(int), st));
    if (P.kind == 2) hipLaunchKernelGGL((mask_small_kernel<1, false>), dim3((unsigned)((P.nBlk + 255) / 256), (unsigned)nframes), dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p, h->dSmall.p, h->dOcc.p);
    else if (P.kind == 1 && P.shift) hipLaunchKernelGGL((mask_small_kernel<4, true>), perBlock, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p, h->dSmall.p, h->dOcc.p);
    else hipLaunchKernelGGL((mask_small_kernel<4, false>), perBlock, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p, h->dSmall.p, h->dOcc.p);
    if (P.kind == 2) hipLaunchKernelGGL(mask_occ_finish_kernel, perBlock, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p, h->dOcc.p, h->dSmall.p);
    const dim3 lumaGrid((unsigned)(((long long)P.segs[0] * ((P.H[0] + MK_ROWS - 1) / MK_ROWS) + 255) / 256), (unsigned)nframes);
    const dim3 chromaGrid((unsigned)(((long long)P.segs[1] * ((P.H[1] + MK_ROWS - 1) / MK_ROWS) + 255) / 256), (unsigned)nframes * 2);
    if (h->bits > 8) { // a lane's segment is 16 samples in either form: the same grids
        hipLaunchKernelGGL((mask_planes_kernel<0, 1>), lumaGrid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p, h->dSmall.p);
        hipLaunchKernelGGL((mask_planes_kernel<1, 1>), chromaGrid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p, h->dSmall.p);
    } else {
        hipLaunchKernelGGL((mask_planes_kernel<0, 0>), lumaGrid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p, h->dSmall.p);
        hipLaunchKernelGGL((mask_planes_kernel<1, 0>), chromaGrid, dim3(256), 0, st, h->dP.p, h->dJobs.p, h->dOver.p, h->dSmall.p);
    }
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}
