// mvx_degrain_n.hip -- mv.DegrainN on gfx950: the block filter of mvx_degrain.hip at a temporal radius of 1..24 (2..48 references), each
// reference weighed against the threshold of its own temporal distance.  What the two share (geometry, windows, creation arguments, the usable
// kernel, block cover, loads) is in mvx_block_shared.h.
//
// The reference's arithmetic is a template over the radius -- Degrain_C<radius> (MVDegrains.h:30-53), useBlock (:192-206), DegrainWeight
// (:184-189), normaliseWeights<radius> (:208-223) -- and only its six registerFunction calls stop at 6.  This file is that template read at
// any radius, inside the frame loop of mvdegrainGetFrame (MVDegrains.cpp:85-330) with overlaps_c / ToPixels (Overlap.cpp:143-158,335-356) in
// the gather form of mvx_degrain.hip: one thread per row of a cell of W samples, which visits the <= 4 blocks covering the cell.
//
// What differs from mvx_degrain.hip is that nothing is sized by the reference count at compile time:
//   plan    per (frame, plane class, block) a LIST of the references whose weight is not 0 -- a 16-byte head (WSrc, count) and then
//           count entries (byte offset of the compensated block in the reference's super plane, normalised weight, reference index) in a
//           slot of fixed stride.  A reference with weight 0 adds nothing to WSum or to a sum (MVDegrains.h:40-48,212-221), so leaving it
//           out changes no result; far references are mostly such, and only the entries that exist are written and read.
//   gather  takes a block's list in chunks of DN_K entries: DN_K rows requested, then multiply-added into sum[W]; window and
//           normalisation once per block after the last chunk.  The reference planes' base pointers (up to 48 per frame and plane) sit in
//           LDS, the per-distance thresholds and the job tables in global memory.
//   out16   (mvx_degrain_n_create_out16) an 8-bit clip written as 16-bit planes: the cell kernel with an output sample type TO of its own.
//           A block's value is the sum before its >> 8, S = WSrc * src + sum of W_r * ref_r (0..65280), which is what the 16-bit arithmetic
//           gives on samples shifted left by 8: (128 + 256 * S) >> 8 = S.  Loads, plan and lists are those of the 8-bit clip.
#include "mvx_block_shared.h"

static_assert(DN_MAX_RADIUS == MVX_DEGRAIN_N_MAX_RADIUS, "radius limit");

#define DN_K 4 // entries per chunk: DN_K loads of one cell row in flight (W = 8 samples of 16 bits: 4 registers each)

// ------------------------------------------------------------------------------------------------ device structs

struct DNParams : BlkGeom {
    int nRefs;
    int recBytes;            // stride of a plan slot: 16 + 8 * (nRefs rounded up to a multiple of DN_K)
    long long thSAD[2][DN_MAX_RADIUS]; // [luma / chroma][distance - 1]
};

struct DNJob { const unsigned char *src[3]; unsigned char *dst[3]; };

struct __attribute__((aligned(16))) DNHead { int wsrc, count, pad[2]; };
struct __attribute__((aligned(8))) DNEntry { unsigned off; short w; unsigned short r; };
static_assert(sizeof(DNHead) == 16 && sizeof(DNEntry) == 8, "plan slot layout");
static int dn_rec_bytes(int nrefs) { return 16 + 8 * ((nrefs + DN_K - 1) / DN_K * DN_K); }

// ------------------------------------------------------------------------------------------------ kernels

// one thread per (job, block): both plane classes' lists.  The references are walked DN_K at a time so that DN_K vector loads are in flight;
// raw weights go into the slot as they are found, and are normalised in place once WSum is known.
__global__ __launch_bounds__(256) void dn_plan_kernel(const DNParams *Pp, const unsigned char *const *blobs, const unsigned *lv0, unsigned char *plan) {
    const DNParams &P = *Pp;
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.nBlk) return;
    const int by = i / P.nBlkX, bx = i - by * P.nBlkX;
    const int n = P.nRefs, ncls = P.nplanes > 1 ? 2 : 1;
    typedef unsigned pl_v4 __attribute__((ext_vector_type(4), aligned(4)));
    unsigned char *slot[2];
    int count[2] = { 0, 0 }, WSum[2] = { dn_wsum_begin(), dn_wsum_begin() };
    for (int c = 0; c < 2; c++) slot[c] = plan + ((size_t)f * 2 + c) * P.nBlk * P.recBytes + (size_t)i * P.recBytes;
    for (int r0 = 0; r0 < n; r0 += DN_K) {
        pl_v4 vv[DN_K]; bool us[DN_K];
#pragma unroll
        for (int k = 0; k < DN_K; k++) {
            const int r = r0 + k;
            const unsigned l0 = r < n ? lv0[f * n + r] : 0u;
            us[k] = l0 != 0u;
            vv[k] = pl_v4{0, 0, 0, 0};
            if (us[k]) vv[k] = *(DG_GL const pl_v4 *)(dg_gl(blobs[f * n + r]) + l0 + (size_t)i * sizeof(GVecD));
        }
#pragma unroll
        for (int k = 0; k < DN_K; k++) {
            if (!us[k]) continue; // MVDegrains.h:192-206 useBlock: weight 0
            const int r = r0 + k;
            const int vx = (int)vv[k][0], vy = (int)vv[k][1];
            const long long sad = (long long)(((unsigned long long)vv[k][3] << 32) | vv[k][2]);
            const int blx = ((bx * P.pl[0].stepX) << P.logPel) + vx, bly = ((by * P.pl[0].stepY) << P.logPel) + vy; // block origin Fakery.c:31-32
            for (int c = 0; c < ncls; c++) {
                const PlaneG &g = P.pl[c];
                const int w = dn_weight(P.thSAD[c][dn_distance(r) - 1], sad);
                if (w == 0) continue;
                DNEntry e;
                e.off = sup_offset(g, P.pel, P.logPel, P.bps, c ? blx >> g.subX : blx, c ? bly >> g.subY : bly);
                e.w = (short)w; e.r = (unsigned short)r;
                ((DNEntry *)(slot[c] + sizeof(DNHead)))[count[c]++] = e;
                WSum[c] += w;
            }
        }
    }
    for (int c = 0; c < ncls; c++) { // MVDegrains.h:208-223 normaliseWeights
        const double scale = dn_scale(WSum[c]);
        DNEntry *e = (DNEntry *)(slot[c] + sizeof(DNHead));
        int WSrc = 256;
        for (int k = 0; k < count[c]; k++) { const int w = dn_scaled(e[k].w, scale); WSrc -= w; e[k].w = (short)w; }
        DNHead h; h.wsrc = WSrc; h.count = count[c]; h.pad[0] = h.pad[1] = 0;
        *(DNHead *)slot[c] = h;
    }
}

typedef unsigned dn_v4 __attribute__((ext_vector_type(4), aligned(16)));

// the cell's row inside one block: Degrain_C (MVDegrains.h:30-53) over the block's list, DN_K entries at a time.  slot: the block's plan slot
// (16-byte aligned), refB: the frame's reference planes in LDS.  The head and the first chunk of entries are requested together (a slot has
// room for at least DN_K entries), and every later chunk before the rows of the one before it are used, so a visit is two dependent round
// trips (list -> rows) whatever the length of the list.  An entry slot past the list's end repeats the chunk's first entry with weight 0, so
// every load goes to an address that a listed reference owns.
template <typename T, int W, int ROUND = 128>
__device__ __forceinline__ void dn_block_sum(DG_GL const unsigned char *slot, const unsigned long long *refB, long long rowOff, const int *s, int *sum) {
    const dn_v4 head = *(DG_GL const dn_v4 *)slot;
    dn_v4 ent[DN_K / 2];
#pragma unroll
    for (int k = 0; k < DN_K / 2; k++) ent[k] = *(DG_GL const dn_v4 *)(slot + sizeof(DNHead) + 16 * k);
    const int wsrc = (int)head[0], count = (int)head[1]; // DNHead
#pragma unroll
    for (int i = 0; i < W; i++) sum[i] = ROUND + s[i] * wsrc;
    for (int e = 0; e < count; e += DN_K) {
        unsigned off[DN_K], wr[DN_K]; // DNEntry: offset, weight | reference << 16
#pragma unroll
        for (int k = 0; k < DN_K; k += 2) { off[k] = ent[k / 2][0]; wr[k] = ent[k / 2][1]; off[k + 1] = ent[k / 2][2]; wr[k + 1] = ent[k / 2][3]; }
        DgRaw<T, W> raw[DN_K];
        int w[DN_K];
#pragma unroll
        for (int k = 0; k < DN_K; k++) {
            const bool valid = e + k < count; // (k == 0 always is)
            const unsigned o = valid ? off[k] : off[0], r = (valid ? wr[k] : wr[0]) >> 16;
            w[k] = valid ? (int)(short)(wr[k] & 0xffffu) : 0;
            raw[k] = dg_load_raw<T, W>(dg_gl((const unsigned char *)refB[r]) + o + rowOff);
        }
        if (e + DN_K < count) {
#pragma unroll
            for (int k = 0; k < DN_K / 2; k++) ent[k] = *(DG_GL const dn_v4 *)(slot + sizeof(DNHead) + (size_t)(e + DN_K) * sizeof(DNEntry) + 16 * k);
        }
#pragma unroll
        for (int k = 0; k < DN_K; k++) {
#pragma unroll
            for (int i = 0; i < W; i++) sum[i] += dg_sample(raw[k], i) * w[k];
        }
    }
}

// One thread per row of a cell: W consecutive samples starting at a multiple of W, where W divides the block width and the block step, so
// that the same blocks cover all of them (blocks side by side: one block).  256 threads = 32 cells x 8 rows of one plane of one job.
// TO: the sample type of the output planes.  TO = T is the reference's filter.  T 8-bit and TO 16-bit is out16: a block's value is its sum S
// without rounding term and shift, the accumulator of the overlap keeps all its 32 bits (S * win <= 65280 * 2048 < 2^31, and the <= 4 terms
// of a sample, whose window weights total 2047..2049, add up to <= 65280 * 2049 / 64 < 2^21), the clamp is at 65535, and the source enters
// the limits and the samples that are passed through as s << 8.
template <typename T, typename TO, int W>
__global__ __launch_bounds__(256) void dn_cell_kernel(const DNParams *Pp, const DNJob *jobs, const unsigned char *const *refs, const unsigned char *plan, int planeFirst, int planesPerFrame) {
    const DNParams &P = *Pp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    constexpr bool OUT16 = sizeof(TO) > sizeof(T);
    constexpr int UP = OUT16 ? 8 : 0; // source sample -> output scale
    __shared__ unsigned long long refB[DN_MAX_REFS];
    if ((int)threadIdx.x < P.nRefs) refB[threadIdx.x] = (unsigned long long)refs[((size_t)f * P.nRefs + threadIdx.x) * 3 + p];
    __syncthreads();
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    const int x0 = c * W;
    if (x0 >= g.W || y >= g.H) return;
    const DNJob &J = jobs[f];
    const unsigned char *srow = J.src[p] + (long long)y * g.srcPitch + (long long)x0 * sizeof(T);
    unsigned char *drow = J.dst[p] + (long long)y * g.dstPitch + (long long)x0 * sizeof(TO);
    const bool fullW = x0 + W <= g.W;
    int s[W];
    if (fullW) dg_load<T, W>(dg_gl(srow), s);
    else {
#pragma unroll
        for (int i = 0; i < W; i++) s[i] = x0 + i < g.W ? (int)((const T *)srow)[i] : 0;
    }
    int out[W];
#pragma unroll
    for (int i = 0; i < W; i++) out[i] = s[i] << UP;
    // MVDegrains.cpp:211-214,238-249,290-298: a plane that is not processed and the strips no block covers keep the source.  The covered
    // width is a multiple of W, so a cell that starts inside it lies inside it (and inside the frame)
    if (g.process && x0 < g.WB && y < g.HB) {
        DG_GL const unsigned char *pl = dg_gl(plan + ((size_t)f * 2 + (p ? 1 : 0)) * P.nBlk * P.recBytes);
        const int pm = OUT16 ? 65535 : (1 << P.bits) - 1;
        int sum[W];
        if (!P.overlap) { // MVDegrains.cpp:238-249: Degrain_C straight into the frame
            const int bx = x0 / g.blkW, by = y / g.blkH;
            const int px = x0 - bx * g.blkW, py = y - by * g.blkH;
            DG_GL const unsigned char *slot = pl + (size_t)(by * P.nBlkX + bx) * P.recBytes;
            dn_block_sum<T, W, OUT16 ? 0 : 128>(slot, refB, (long long)py * g.supPitch + (long long)px * sizeof(T), s, sum);
#pragma unroll
            for (int i = 0; i < W; i++) out[i] = OUT16 ? sum[i] : (int)(T)(sum[i] >> 8);
        } else {
            // blocks covering this cell: bx in [bx0, bx1], by in [by0, by1]
            int bx0, bx1, by0, by1;
            blk_cover(x0, g.blkW, g.stepX, P.nBlkX, bx0, bx1);
            blk_cover(y, g.blkH, g.stepY, P.nBlkY, by0, by1);
            unsigned acc[W];
#pragma unroll
            for (int i = 0; i < W; i++) acc[i] = 0;
            const int16_t *win = P.win[p];
            for (int by = by0; by <= by1; by++) {
                const int py = y - by * g.stepY;
                const int wby = BLK_WIN_ROW(by, P.nBlkY);
                for (int bx = bx0; bx <= bx1; bx++) {
                    const int px = x0 - bx * g.stepX; // 0 <= px <= blkW - W
                    const int wbx = BLK_WIN_COL(bx, P.nBlkX);
                    DG_GL const unsigned char *slot = pl + (size_t)(by * P.nBlkX + bx) * P.recBytes;
                    const DgRaw<unsigned short, W> wr = dg_load_raw<unsigned short, W>(dg_gl((const unsigned char *)(win + (wby + wbx) * g.blkW * g.blkH + py * g.blkW + px)));
                    dn_block_sum<T, W, OUT16 ? 0 : 128>(slot, refB, (long long)py * g.supPitch + (long long)px * sizeof(T), s, sum);
#pragma unroll
                    for (int i = 0; i < W; i++) { // overlaps_c, Overlap.cpp:143-158
                        const int val = OUT16 ? sum[i] : (int)(T)(sum[i] >> 8);
                        acc[i] += (unsigned)((val * dg_sample(wr, i)) >> 6);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < W; i++) {
                unsigned a0 = acc[i];
                if (sizeof(T) == 1 && !OUT16) a0 &= 0xffffu; // 16-bit accumulator of the 8-bit path (Overlap.cpp:254-256)
                const int a = (int)((a0 + 16) >> 5); // ToPixels, Overlap.cpp:335-356
                out[i] = a > pm ? pm : a;
            }
        }
        if (g.limit < pm) { // LimitChanges, MVDegrains.h:163-181
#pragma unroll
            for (int i = 0; i < W; i++) {
                const int lo = (s[i] << UP) - g.limit, hi = (s[i] << UP) + g.limit;
                out[i] = out[i] < lo ? lo : out[i];
                out[i] = out[i] > hi ? hi : out[i];
            }
        }
    }
    if (fullW) dg_store<TO, W>(dg_glw(drow), out);
    else {
#pragma unroll
        for (int i = 0; i < W; i++) if (x0 + i < g.W) ((TO *)drow)[i] = (TO)out[i];
    }
}

// ---- float clips (mvx_degrain_n_create_float): the cell kernel with a float accumulator.  Plan, lists, usable pass and the structure of the
// gather are those above; the arithmetic is float32, every operation rounded on its own (include/mvtools_amd.h).

// a block's value at the cell's row: V = (WSrc * s + w_1 * ref_1 + ... in list order) * (1 / 256).  An entry slot past the list's end is
// loaded like dn_block_sum's (the chunk's first entry) and then left out by a select: nothing is added for it.
template <int W>
__device__ __forceinline__ void dn_block_value_float(DG_GL const unsigned char *slot, const unsigned long long *refB, long long rowOff, const float *s, float *V) {
    const dn_v4 head = *(DG_GL const dn_v4 *)slot;
    dn_v4 ent[DN_K / 2];
#pragma unroll
    for (int k = 0; k < DN_K / 2; k++) ent[k] = *(DG_GL const dn_v4 *)(slot + sizeof(DNHead) + 16 * k);
    const int wsrc = (int)head[0], count = (int)head[1]; // DNHead
    float S[W];
#pragma unroll
    for (int i = 0; i < W; i++) S[i] = (float)wsrc * s[i];
    for (int e = 0; e < count; e += DN_K) {
        unsigned off[DN_K], wr[DN_K];
#pragma unroll
        for (int k = 0; k < DN_K; k += 2) { off[k] = ent[k / 2][0]; wr[k] = ent[k / 2][1]; off[k + 1] = ent[k / 2][2]; wr[k + 1] = ent[k / 2][3]; }
        DgRaw<float, W> raw[DN_K];
        float w[DN_K];
        bool valid[DN_K];
#pragma unroll
        for (int k = 0; k < DN_K; k++) {
            valid[k] = e + k < count; // (k == 0 always is)
            const unsigned o = valid[k] ? off[k] : off[0], r = (valid[k] ? wr[k] : wr[0]) >> 16;
            w[k] = (float)(int)(short)(wr[k] & 0xffffu);
            raw[k] = dg_load_raw<float, W>(dg_gl((const unsigned char *)refB[r]) + o + rowOff);
        }
        if (e + DN_K < count) {
#pragma unroll
            for (int k = 0; k < DN_K / 2; k++) ent[k] = *(DG_GL const dn_v4 *)(slot + sizeof(DNHead) + (size_t)(e + DN_K) * sizeof(DNEntry) + 16 * k);
        }
#pragma unroll
        for (int k = 0; k < DN_K; k++) {
#pragma unroll
            for (int i = 0; i < W; i++) {
                const float t = S[i] + w[k] * __uint_as_float(raw[k].d[i]);
                S[i] = valid[k] ? t : S[i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) V[i] = S[i] * (1.0f / 256.0f);
}

// dn_cell_kernel's cells and threads.  overlap > 0: acc = acc + V * win over the covering blocks (by outer, bx inner, ascending), divided by the
// integer sum of those window weights (2047..2049), so that a flat area stays flat.  limit is on the 8-bit scale: L = limit / 255.  lv0: the
// usable pass's result; a job none of whose references is usable keeps its source bit for bit (with overlap acc / wsum would not).
template <int W>
__global__ __launch_bounds__(256) void dn_cell_float_kernel(const DNParams *Pp, const DNJob *jobs, const unsigned char *const *refs, const unsigned *lv0, const unsigned char *plan,
                                                            int planeFirst, int planesPerFrame) {
    const DNParams &P = *Pp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    __shared__ unsigned long long refB[DN_MAX_REFS];
    __shared__ int anyUsable;
    if (threadIdx.x == 0) anyUsable = 0;
    __syncthreads();
    if ((int)threadIdx.x < P.nRefs) {
        refB[threadIdx.x] = (unsigned long long)refs[((size_t)f * P.nRefs + threadIdx.x) * 3 + p];
        if (lv0[f * P.nRefs + threadIdx.x] != 0u) anyUsable = 1;
    }
    __syncthreads();
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    const int x0 = c * W;
    if (x0 >= g.W || y >= g.H) return;
    const DNJob &J = jobs[f];
    const unsigned char *srow = J.src[p] + (long long)y * g.srcPitch + (long long)x0 * sizeof(float);
    unsigned char *drow = J.dst[p] + (long long)y * g.dstPitch + (long long)x0 * sizeof(float);
    const bool fullW = x0 + W <= g.W;
    float s[W];
    if (fullW) {
        const DgRaw<float, W> r = dg_load_raw<float, W>(dg_gl(srow));
#pragma unroll
        for (int i = 0; i < W; i++) s[i] = __uint_as_float(r.d[i]);
    } else {
#pragma unroll
        for (int i = 0; i < W; i++) s[i] = x0 + i < g.W ? ((const float *)srow)[i] : 0.0f;
    }
    float out[W];
#pragma unroll
    for (int i = 0; i < W; i++) out[i] = s[i];
    if (g.process && anyUsable && x0 < g.WB && y < g.HB) { // the covered width is a multiple of W: a cell that starts inside it lies inside it
        DG_GL const unsigned char *pl = dg_gl(plan + ((size_t)f * 2 + (p ? 1 : 0)) * P.nBlk * P.recBytes);
        float V[W];
        if (!P.overlap) {
            const int bx = x0 / g.blkW, by = y / g.blkH;
            const int px = x0 - bx * g.blkW, py = y - by * g.blkH;
            DG_GL const unsigned char *slot = pl + (size_t)(by * P.nBlkX + bx) * P.recBytes;
            dn_block_value_float<W>(slot, refB, (long long)py * g.supPitch + (long long)px * sizeof(float), s, V);
#pragma unroll
            for (int i = 0; i < W; i++) out[i] = V[i];
        } else {
            int bx0, bx1, by0, by1;
            blk_cover(x0, g.blkW, g.stepX, P.nBlkX, bx0, bx1);
            blk_cover(y, g.blkH, g.stepY, P.nBlkY, by0, by1);
            float acc[W];
            int wsum[W];
#pragma unroll
            for (int i = 0; i < W; i++) { acc[i] = 0.0f; wsum[i] = 0; }
            const int16_t *win = P.win[p];
            for (int by = by0; by <= by1; by++) {
                const int py = y - by * g.stepY;
                const int wby = BLK_WIN_ROW(by, P.nBlkY);
                for (int bx = bx0; bx <= bx1; bx++) {
                    const int px = x0 - bx * g.stepX; // 0 <= px <= blkW - W
                    const int wbx = BLK_WIN_COL(bx, P.nBlkX);
                    DG_GL const unsigned char *slot = pl + (size_t)(by * P.nBlkX + bx) * P.recBytes;
                    const DgRaw<unsigned short, W> wr = dg_load_raw<unsigned short, W>(dg_gl((const unsigned char *)(win + (wby + wbx) * g.blkW * g.blkH + py * g.blkW + px)));
                    dn_block_value_float<W>(slot, refB, (long long)py * g.supPitch + (long long)px * sizeof(float), s, V);
#pragma unroll
                    for (int i = 0; i < W; i++) {
                        const int wi = dg_sample(wr, i);
                        acc[i] = acc[i] + V[i] * (float)wi;
                        wsum[i] += wi;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < W; i++) out[i] = acc[i] / (float)wsum[i];
        }
        if (g.limit < 255) {
            const float L = (float)g.limit / 255.0f;
#pragma unroll
            for (int i = 0; i < W; i++) out[i] = fmaxf(s[i] - L, fminf(s[i] + L, out[i]));
        }
    }
    if (fullW) {
        DG_GL unsigned char *d = dg_glw(drow);
        if constexpr (W >= 4) {
#pragma unroll
            for (int k = 0; k < W / 4; k++) { dg_uv4 t = { __float_as_uint(out[4 * k]), __float_as_uint(out[4 * k + 1]), __float_as_uint(out[4 * k + 2]), __float_as_uint(out[4 * k + 3]) }; *(DG_GL dg_uv4 *)(d + 16 * k) = t; }
        } else if constexpr (W == 2) { dg_uv2 t = { __float_as_uint(out[0]), __float_as_uint(out[1]) }; *(DG_GL dg_uv2 *)d = t; }
        else *(DG_GL dg_uv1 *)d = __float_as_uint(out[0]);
    } else {
#pragma unroll
        for (int i = 0; i < W; i++) if (x0 + i < g.W) ((float *)drow)[i] = out[i];
    }
}

// ------------------------------------------------------------------------------------------------ host object

struct mvx_degrain_n {
    CallGuard guard;
    DNParams P;
    mvx_degrain_n_info info;
    DevBuf<DNParams> dP;
    DevBuf<unsigned char> dTables;   // per call: the jobs, then the reference planes [job][reference][plane], then the blobs [job][reference]
    DevBuf<unsigned> dLv0;
    DevBuf<unsigned char> dPlan;
    BlkWin win;
    bool out16 = false;              // 8-bit clip, 16-bit output planes
    bool flt = false;                // float clip, float super clip, float output planes
};

static int dn_create(const mvx_degrain_n_args *a, const mvx_analysis_data *ad, const mvx_super *sup, const ptrdiff_t src_pitch[3], const ptrdiff_t super_pitch[3],
                     const ptrdiff_t dst_pitch[3], int kind, mvx_degrain_n **out, char *err) {
    MVX_CREATE_BEGIN(out);
    if (kind != DG_FLOAT) MVX_REFUSE_FLOAT(sup, "DegrainN");
    const mvx_super_info &si = sup->info;
    const int radius = a->radius;
    const char *name = "DegrainN";
    if (radius < 1 || radius > MVX_DEGRAIN_N_MAX_RADIUS) MVX_FAIL("%s: radius must be between 1 and %d.", name, MVX_DEGRAIN_N_MAX_RADIUS);
    DgResolved r;
    if (int rc = dg_resolve(name, a, kind, ad, si, &r, err)) return rc;
    mvx_degrain_n *h;
    if (int rc = blk_new(&h, ad, si, src_pitch, super_pitch, dst_pitch, err, "src", kind == DG_OUT16 ? 2 : 0)) return rc;
    h->info = r.info;
    h->out16 = kind == DG_OUT16;
    h->flt = kind == DG_FLOAT;
    DNParams &P = h->P;
    P.nRefs = 2 * radius; P.recBytes = dn_rec_bytes(P.nRefs);
    for (int d = 0; d < radius; d++) { P.thSAD[0][d] = r.info.thsad_d[d]; P.thSAD[1][d] = r.info.thsadc_d[d]; }
    dg_apply(P, r, si);
    *out = h;
    return MVX_OK;
}

extern "C" __attribute__((visibility("default"))) int mvx_degrain_n_create(const mvx_degrain_n_args *a, const mvx_analysis_data *ad, const mvx_super *sup, const ptrdiff_t src_pitch[3],
                                    const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3], mvx_degrain_n **out, char *err) {
    return dn_create(a, ad, sup, src_pitch, super_pitch, dst_pitch, DG_PLAIN, out, err);
}
extern "C" __attribute__((visibility("default"))) int mvx_degrain_n_create_out16(const mvx_degrain_n_args *a, const mvx_analysis_data *ad, const mvx_super *sup, const ptrdiff_t src_pitch[3],
                                    const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3], mvx_degrain_n **out, char *err) {
    return dn_create(a, ad, sup, src_pitch, super_pitch, dst_pitch, DG_OUT16, out, err);
}
extern "C" __attribute__((visibility("default"))) int mvx_degrain_n_create_float(const mvx_degrain_n_args *a, const mvx_analysis_data *ad, const mvx_super *sup, const ptrdiff_t src_pitch[3],
                                    const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3], mvx_degrain_n **out, char *err) {
    return dn_create(a, ad, sup, src_pitch, super_pitch, dst_pitch, DG_FLOAT, out, err);
}
extern "C" __attribute__((visibility("default"))) int mvx_degrain_n_out_bits(const mvx_degrain_n *d) { return d->flt ? 32 : d->out16 ? 16 : d->P.bits; }

extern "C" __attribute__((visibility("default"))) void mvx_degrain_n_get_info(const mvx_degrain_n *d, mvx_degrain_n_info *info) { *info = d->info; }
extern "C" __attribute__((visibility("default"))) void mvx_degrain_n_destroy(mvx_degrain_n *d) { delete d; }

template <typename T, typename TO> static void dn_launch_cells(int W, dim3 grid, hipStream_t st, const DNParams *dP, const DNJob *dJ, const unsigned char *const *dRefs, const unsigned char *plan, int p0, int npl) {
#define DNC(N) hipLaunchKernelGGL((dn_cell_kernel<T, TO, N>), grid, dim3(256), 0, st, dP, dJ, dRefs, plan, p0, npl)
    switch (W) { case 1: DNC(1); break; case 2: DNC(2); break; case 4: DNC(4); break; default: DNC(8); break; }
#undef DNC
}

extern "C" __attribute__((visibility("default"))) int mvx_degrain_n_frames(mvx_degrain_n *d, int nframes, const mvx_degrain_n_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    const DNParams &P = d->P;
    const size_t n = (size_t)nframes, nr = (size_t)P.nRefs;
    for (size_t f = 0; f < n; f++) {
        const mvx_degrain_n_job &J = jobs[f];
        if (!J.refs || !J.blobs) { mvx_set_error("mvx_degrain_n_frames: a job needs its reference table and its blob table"); return MVX_E_ARG; }
        if (int rc = fps_check_planes("mvx_degrain_n_frames", "src", J.src, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_degrain_n_frames", "dst", J.dst, P.nplanes, d->out16 ? 2 : P.bps, true)) return rc;
        for (size_t r = 0; r < nr; r++)
            if (int rc = fps_check_planes("mvx_degrain_n_frames", "reference super", J.refs[r], P.nplanes, 16, false)) return rc;
    }
    CallGuard::Scope scope(d->guard, st);
    int rc = blk_upload(d->dP, d->P, d->win);
    if (rc) return rc;
    // one host block, one copy: jobs | reference planes | blobs (each part a multiple of 8 bytes)
    const size_t offRefs = sizeof(DNJob) * n, offBlobs = offRefs + sizeof(void *) * 3 * nr * n, total = offBlobs + sizeof(void *) * nr * n;
    std::vector<unsigned char> host(total, 0);
    DNJob *hj = (DNJob *)host.data();
    const unsigned char **hr = (const unsigned char **)(host.data() + offRefs), **hb = (const unsigned char **)(host.data() + offBlobs);
    for (size_t f = 0; f < n; f++) {
        for (int p = 0; p < 3; p++) { hj[f].src[p] = (const unsigned char *)jobs[f].src[p]; hj[f].dst[p] = (unsigned char *)jobs[f].dst[p]; }
        for (size_t r = 0; r < nr; r++) {
            for (int p = 0; p < 3; p++) hr[(f * nr + r) * 3 + p] = (const unsigned char *)jobs[f].refs[r][p];
            hb[f * nr + r] = (const unsigned char *)jobs[f].blobs[r];
        }
    }
    const size_t planBytes = (size_t)P.recBytes * 2 * P.nBlk * n;
    HIP_CHECK(d->dTables.reserve(total, total));
    HIP_CHECK(d->dLv0.reserve(nr * n, nr * n));
    HIP_CHECK(d->dPlan.reserve(planBytes, planBytes / 2));
    HIP_CHECK(hipMemcpyAsync(d->dTables.p, host.data(), total, hipMemcpyHostToDevice, st));
    const DNJob *dJ = (const DNJob *)d->dTables.p;
    const unsigned char *const *dRefs = (const unsigned char *const *)(d->dTables.p + offRefs), *const *dBlobs = (const unsigned char *const *)(d->dTables.p + offBlobs);
    hipLaunchKernelGGL(blk_usable_kernel<DNParams>, dim3(P.nRefs, nframes), dim3(256), 0, st, d->dP.p, P.nRefs, BlkTables{dRefs, dBlobs}, d->dLv0.p);
    hipLaunchKernelGGL(dn_plan_kernel, dim3((P.nBlk + 255) / 256, nframes), dim3(256), 0, st, d->dP.p, dBlobs, d->dLv0.p, d->dPlan.p);
    for (int cls = 0; cls < (P.nplanes > 1 ? 2 : 1); cls++) { // one launch for the luma planes of all jobs, one for both chroma planes
        const int p0 = cls, npl = cls ? 2 : 1, W = blk_cell_width(P.pl[p0], 8);
        const dim3 grid(((P.pl[p0].W + W - 1) / W + 31) / 32, (P.pl[p0].H + 7) / 8, nframes * npl);
        if (d->flt) {
#define DNF(N) hipLaunchKernelGGL((dn_cell_float_kernel<N>), grid, dim3(256), 0, st, d->dP.p, dJ, dRefs, d->dLv0.p, d->dPlan.p, p0, npl)
            switch (W) { case 1: DNF(1); break; case 2: DNF(2); break; case 4: DNF(4); break; default: DNF(8); break; }
#undef DNF
        } else if (d->out16) dn_launch_cells<uint8_t, uint16_t>(W, grid, st, d->dP.p, dJ, dRefs, d->dPlan.p, p0, npl);
        else if (P.bps == 1) dn_launch_cells<uint8_t, uint8_t>(W, grid, st, d->dP.p, dJ, dRefs, d->dPlan.p, p0, npl);
        else dn_launch_cells<uint16_t, uint16_t>(W, grid, st, d->dP.p, dJ, dRefs, d->dPlan.p, p0, npl);
    }
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}
