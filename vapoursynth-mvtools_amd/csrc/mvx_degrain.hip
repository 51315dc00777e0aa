// mvx_degrain.hip -- mv.Degrain1..6 on gfx950, with the overlap windows, mvx_vectors_size and mvx_scale_thscd that every vector consumer uses, and
// mv.SCDetection at the end under its own heading.  What Degrain shares with DegrainN, Compensate, CompensateN and BlockFPS (mvx_degrain_n.hip,
// mvx_compensate.hip, mvx_blockfps.hip) is in mvx_block_shared.h, what they share with the flow filters and mv.Mask in mvx_fps_shared.h.
//
// The reference walks blocks, blends each block into a temp (Degrain_C, MVDegrains.h:30-53), scatters it times a
// raised-cosine window into a 16/32-bit accumulator (overlaps_c, Overlap.cpp:143-158) and finally normalises
// (ToPixels, Overlap.cpp:335-356).  The accumulator never saturates, so the sum is order-free and the GPU form is
// a GATHER: one thread per output sample visits the <=4 blocks covering it, recomputes that block's blended sample
// and accumulates it times the window tap.  No accumulator plane, no atomics, one pass over HBM:
//   plan kernel   : per (frame, block) -> per-reference weights (fp64 exactly as MVDegrains.h:184-223) and the byte
//                   offset of the motion-compensated block inside the reference super frame (MVDegrains.h:192-206)
//   gather kernel : per output sample  -> blend + window + normalise + uncovered strips + LimitChanges.
#include "mvx_block_shared.h"

#define MOTION_USE_CHROMA_MOTION 8

// ------------------------------------------------------------------------------------------------ host helpers

// Overlap.cpp:40-125 overInit.  M_PI is the double constant; the cosf argument is formed in double.
static void win1d(float *w, float *first, float *last, int n, int o) {
    for (int i = 0; i < o; i++) {
        w[i] = cosf((float)(M_PI * (i - o + 0.5f) / (o * 2)));
        w[i] = w[i] * w[i];
        first[i] = 1; last[i] = w[i];
    }
    for (int i = o; i < n - o; i++) { w[i] = 1; first[i] = 1; last[i] = 1; }
    for (int i = n - o; i < n; i++) {
        w[i] = cosf((float)(M_PI * (i - n + o + 0.5f) / (o * 2)));
        w[i] = w[i] * w[i];
        first[i] = w[i]; last[i] = 1;
    }
}

void mvx_over_windows(int16_t *win9, int nx, int ny, int ox, int oy) {
    std::vector<float> fx(nx * 3), fy(ny * 3);
    win1d(&fx[0], &fx[nx], &fx[2 * nx], nx, ox);
    win1d(&fy[0], &fy[ny], &fy[2 * ny], ny, oy);
    const float *x[3] = { &fx[nx], &fx[0], &fx[2 * nx] }; // first, middle, last
    const float *y[3] = { &fy[ny], &fy[0], &fy[2 * ny] };
    for (int wy = 0; wy < 3; wy++)
        for (int wx = 0; wx < 3; wx++) {
            int16_t *w = win9 + nx * ny * (wy * 3 + wx);
            for (int j = 0; j < ny; j++)
                for (int i = 0; i < nx; i++) w[j * nx + i] = (int16_t)(int)(y[wy][j] * x[wx][i] * 2048 + 0.5f);
        }
}

extern "C" __attribute__((visibility("default"))) int mvx_vectors_size(const mvx_analysis_data *ad) { // Fakery.c:110-121, GroupOfPlanes.c:127-148
    const int nWidth_B = (ad->nBlkSizeX - ad->nOverlapX) * ad->nBlkX + ad->nOverlapX;
    const int nHeight_B = (ad->nBlkSizeY - ad->nOverlapY) * ad->nBlkY + ad->nOverlapY;
    int size = 8;
    for (int i = ad->nLvCount - 1; i >= 0; i--) {
        const int bx = ((nWidth_B >> i) - ad->nOverlapX) / (ad->nBlkSizeX - ad->nOverlapX);
        const int by = ((nHeight_B >> i) - ad->nOverlapY) / (ad->nBlkSizeY - ad->nOverlapY);
        size += 4 + bx * by * 16;
    }
    return size;
}

extern "C" __attribute__((visibility("default"))) void mvx_scale_thscd(int64_t *thscd1, int32_t *thscd2, const mvx_analysis_data *ad) { // MVAnalysisData.c:7-31
    *thscd1 = *thscd1 * (ad->nBlkSizeX * ad->nBlkSizeY) / (8 * 8);
    if (ad->nMotionFlags & MOTION_USE_CHROMA_MOTION) *thscd1 += *thscd1 / (ad->xRatioUV * ad->yRatioUV) * 2;
    const int pixelMax = (1 << ad->bitsPerSample) - 1;
    *thscd1 = (int64_t)((double)*thscd1 * pixelMax / 255.0 + 0.5);
    *thscd2 = *thscd2 * ad->nBlkX * ad->nBlkY / 256;
}

// ------------------------------------------------------------------------------------------------ shared device structs

struct DGParams : BlkGeom {
    int nRefs;
    long long thSAD[2];
};

struct DGJob {
    const unsigned char *src[3];
    const unsigned char *refs[12][3];
    const unsigned char *blobs[12];
    unsigned char *dst[3];
};

// plan record: one per (frame, plane class luma/chroma, block), sized for the filter's 2 * radius references (Degrain3: 40 bytes; a fixed
// 12-reference record was 76 -- at 4K16 the plan of a 512-frame batch was 10 GB written and read back, more than the vector blobs it digests)
template <int NR> struct PlanRecT {
    unsigned off[NR];  // byte offset of the compensated block's first sample inside the reference super plane
    short w[NR];
    short wsrc;
    short pad;
};
static size_t plan_rec_bytes(int nrefs) { return (size_t)6 * nrefs + 4; }
static_assert(sizeof(PlanRecT<6>) == 40 && sizeof(PlanRecT<12>) == 76 && sizeof(PlanRecT<2>) == 16, "plan record layout");

// ------------------------------------------------------------------------------------------------ kernels

// per (job, reference): fgopIsUsable of the reference's vectors, 0 for a reference frame outside the clip (which may have no blob at all)
__global__ __launch_bounds__(256) void usable_kernel(const DGParams *Pp, const DGJob *jobs, int *usable) {
    const DGParams &P = *Pp;
    const int f = blockIdx.y, r = blockIdx.x;
    const bool ok = fps_block_usable(jobs[f].blobs[r], jobs[f].refs[r][0] != nullptr, P.nLvCount, P.nBlk, P.thscd1, P.thscd2);
    if (threadIdx.x == 0) usable[f * 12 + r] = ok;
}

// (r6: left alone the register allocator takes 162 registers for six references -- three waves per SIMD; asked for six it needs 71 and spills nothing:
// 4.41 -> 2.78 ms per 341 4K16 frames, profiles/r6_degrain_window_plan_ab.txt)
constexpr int dg_plan_waves(int nr) { return nr <= 6 ? 6 : 4; }
template <int NR>
__global__ __launch_bounds__(256, dg_plan_waves(NR)) void degrain_plan_kernel(const DGParams *Pp, const DGJob *jobs, const int *usable, PlanRecT<NR> *plan) {
    typedef PlanRecT<NR> PlanRec;
    const DGParams &P = *Pp;
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const DGJob &J = jobs[f];
    constexpr int n = NR; // (= P.nRefs)
    // where level 0 starts inside each blob: found once per workgroup (a walk over the per-level size headers: nLvCount - 1 dependent loads), not
    // once per thread and reference (r4); the vectors themselves through global-address-space pointers, all requested before the first is used
    __shared__ unsigned lv0[NR];
    if (threadIdx.x < NR) lv0[threadIdx.x] = usable[f * 12 + threadIdx.x] ? (unsigned)((const unsigned char *)mvx_level0(J.blobs[threadIdx.x], P.nLvCount) - J.blobs[threadIdx.x]) : 0u;
    __syncthreads();
    if (i >= P.nBlk) return;
    const int by = i / P.nBlkX, bx = i - by * P.nBlkX;
    int vx[NR], vy[NR]; long long sad[NR]; int us[NR];
    typedef unsigned pl_v4 __attribute__((ext_vector_type(4), aligned(4)));
    pl_v4 vv[NR];
#pragma unroll
    for (int r = 0; r < n; r++) {
        us[r] = usable[f * 12 + r];
        vv[r] = pl_v4{0, 0, 0, 0};
        if (us[r]) vv[r] = *(DG_GL const pl_v4 *)(dg_gl(J.blobs[r]) + lv0[r] + (size_t)i * sizeof(GVecD)); // (a reference that is not usable may have no blob at all)
    }
#pragma unroll
    for (int r = 0; r < n; r++) { vx[r] = (int)vv[r][0]; vy[r] = (int)vv[r][1]; sad[r] = (long long)(((unsigned long long)vv[r][3] << 32) | vv[r][2]); }
    const int ncls = P.nplanes > 1 ? 2 : 1;
    for (int c = 0; c < ncls; c++) {
        const PlaneG &g = P.pl[c];
        PlanRec rec;
        int W[NR], WSum = 256 + 1;
        for (int r = 0; r < n; r++) {
            W[r] = 0; rec.off[r] = 0;
            if (us[r]) { // MVDegrains.h:192-200 useBlock; block origin Fakery.c:31-32
                const int blx = ((bx * P.pl[0].stepX) << P.logPel) + vx[r], bly = ((by * P.pl[0].stepY) << P.logPel) + vy[r];
                rec.off[r] = sup_offset(g, P.pel, P.logPel, P.bps, c ? blx >> g.subX : blx, c ? bly >> g.subY : bly);
                // a block that starts at an odd sample is read from the shifted copy, where it starts at a dword-aligned address: same samples, but a
                // wave's 16-byte loads at 2-byte-aligned addresses cost the texture addresser 64 cycles instead of 16 (tools/micro/ta_pattern.hip, patterns
                // 21 / 22), and these loads keep it busy 78 % of the kernel's run time (profiles/r4_stream_kernel_counters.txt)
                if (g.shadow && (rec.off[r] & 2u)) rec.off[r] = (rec.off[r] & ~3u) + (unsigned)g.shadow;
                W[r] = dn_weight(P.thSAD[g.thIdx], sad[r]); // MVDegrains.h:184-189
            }
            WSum += W[r];
        }
        const double scale = 256.0 / WSum; // MVDegrains.h:208-223 normaliseWeights
        int WSrc = 256;
        for (int r = 0; r < n; r++) { W[r] = (int)(W[r] * scale); WSrc -= W[r]; rec.w[r] = (short)W[r]; }
        rec.wsrc = (short)WSrc; rec.pad = 0;
        plan[((size_t)f * 2 + c) * P.nBlk + i] = rec;
    }
}

template <typename T, int NR>
__global__ __launch_bounds__(256) void degrain_kernel(const DGParams *Pp, const DGJob *jobs, const PlanRecT<NR> *plan) {
    typedef PlanRecT<NR> PlanRec;
    const DGParams &P = *Pp;
    const int z = blockIdx.z, f = z / 3, p = z % 3;
    if (p >= P.nplanes) return;
    const PlaneG &g = P.pl[p];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const DGJob &J = jobs[f];
    const T *srow = (const T *)(J.src[p] + (long long)y * g.srcPitch);
    T *drow = (T *)(J.dst[p] + (long long)y * g.dstPitch);
    const int s = srow[x];
    if (!g.process || x >= g.WB || y >= g.HB) { drow[x] = (T)s; return; } // MVDegrains.cpp:211-214,238-249,290-298
    const PlanRec *pl = plan + ((size_t)f * 2 + (p ? 1 : 0)) * P.nBlk;
    int out;
    if (!P.overlap) {
        const int bx = x / g.blkW, by = y / g.blkH;
        const int px = x - bx * g.blkW, py = y - by * g.blkH;
        const PlanRec &R = pl[by * P.nBlkX + bx];
        int sum = 128 + s * R.wsrc;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int w = R.w[r];
            if (w) sum += (int)((const T *)(J.refs[r][p] + R.off[r] + (long long)py * g.supPitch))[px] * w;
        }
        out = (T)(sum >> 8);
    } else {
        // blocks covering this sample: bx in [bx0, bx1], by in [by0, by1]
        int bx0, bx1, by0, by1;
        blk_cover(x, g.blkW, g.stepX, P.nBlkX, bx0, bx1);
        blk_cover(y, g.blkH, g.stepY, P.nBlkY, by0, by1);
        unsigned acc = 0;
        const int16_t *win = P.win[p];
        for (int by = by0; by <= by1; by++) {
            const int py = y - by * g.stepY;
            const int wby = BLK_WIN_ROW(by, P.nBlkY);
            for (int bx = bx0; bx <= bx1; bx++) {
                const int px = x - bx * g.stepX;
                const int wbx = BLK_WIN_COL(bx, P.nBlkX);
                const PlanRec &R = pl[by * P.nBlkX + bx];
                int sum = 128 + s * R.wsrc;
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const int w = R.w[r];
                    if (w) sum += (int)((const T *)(J.refs[r][p] + R.off[r] + (long long)py * g.supPitch))[px] * w;
                }
                const int val = (T)(sum >> 8);
                acc += (unsigned)((val * (int)win[(wby + wbx) * g.blkW * g.blkH + py * g.blkW + px]) >> 6);
            }
        }
        if (sizeof(T) == 1) acc &= 0xffffu; // 16-bit accumulator of the 8-bit path (Overlap.cpp:254-256); never overflows in practice
        const int a = (int)((acc + 16) >> 5); // Overlap.cpp:335-356
        const int pm = (1 << P.bits) - 1;
        out = a > pm ? pm : a;
    }
    if (g.limit < (1 << P.bits) - 1) { // MVDegrains.h:163-181
        int lo = s - g.limit, hi = s + g.limit;
        out = out < lo ? lo : out;
        out = out > hi ? hi : out;
    }
    drow[x] = (T)out;
}

// ---- vectorised gather for overlapped blocks: one thread per row of an overlap cell.
// A cell is stepX consecutive samples starting at a multiple of stepX: all of them are covered by the same <= 2 x 2
// blocks, and inside one block they are contiguous, so every (block, reference) costs ONE unaligned vector load of
// W = stepX samples instead of W scalar loads, and the plan record / window row are fetched once per W outputs.
// Same arithmetic per sample as degrain_kernel (Degrain_C + overlaps_c + ToPixels + LimitChanges).
// Pointers that come out of the job tables are generic ("flat") to the compiler; flat loads are slower and every one of them is waited
// for with vmcnt(0) lgkmcnt(0).  The vector helpers therefore take global-address-space pointers (dg_gl casts).
// r5: the weighted sum of TWO references per instruction for 16-bit samples (MVDegrains.h:31-53: sum += ref * W, all terms non-negative and < 2^24):
// v_perm_b32 pairs sample i of reference a with sample i of reference b, v_dot2_u32_u16 multiplies the pair by the two weights and adds.  Per sample and pair of
// references 2 instructions instead of 4 (two shifts / masks + two multiply-adds); same integers.
typedef unsigned short dg_us2 __attribute__((ext_vector_type(2)));
template <int W> __device__ __forceinline__ void dg_mad_pair_u16(const DgRaw<unsigned short, W> &a, const DgRaw<unsigned short, W> &b, int wa, int wb, int *sum) {
    const dg_us2 w = { (unsigned short)wa, (unsigned short)wb };
#pragma unroll
    for (int j = 0; j < (W + 1) / 2; j++) {
        const unsigned lo = __builtin_amdgcn_perm(b.d[j], a.d[j], 0x05040100u); // (a[2j], b[2j])
        sum[2 * j] = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(dg_us2, lo), w, (unsigned)sum[2 * j], false);
        if (2 * j + 1 < W) {
            const unsigned hi = __builtin_amdgcn_perm(b.d[j], a.d[j], 0x07060302u); // (a[2j + 1], b[2j + 1])
            sum[2 * j + 1] = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(dg_us2, hi), w, (unsigned)sum[2 * j + 1], false);
        }
    }
}
// the weighted references of one block into sum[]: pairs of references for 16-bit samples (NR is even: 2 x radius), one at a time otherwise
template <typename T, int NR, int W, typename REC> __device__ __forceinline__ void dg_mad_refs(const DgRaw<T, W> *raw, const REC &R, int *sum) {
    if constexpr (sizeof(T) == 2 && NR % 2 == 0) {
#pragma unroll
        for (int r = 0; r < NR; r += 2) dg_mad_pair_u16<W>(raw[r], raw[r + 1], R.w[r], R.w[r + 1], sum);
    } else {
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int w = R.w[r];
#pragma unroll
            for (int i = 0; i < W; i++) sum[i] += dg_sample<T, W>(raw[r], i) * w;
        }
    }
}

#define DG_TILE_MAX (34 * 6) // plan records of a workgroup's tile (32 cells x 8 rows): 33 block columns x at most 6 block rows (2-sample cell rows: five)
// blocks of blkW x blkH stepping by stepX x stepY: the records that cover 32 cells x 8 rows fit the tile (always, for the geometries the cell kernel is launched on:
// a power-of-two step below the block size is half the block size)
constexpr bool dg_tiled(int nrefs) { return nrefs >= 6; }
static bool dg_tile_fits(int blkW, int blkH, int stepX, int stepY) { return (31 + (blkW + stepX - 1) / stepX) * (7 / stepY + (blkH + stepY - 1) / stepY + 1) <= DG_TILE_MAX; }
// (4-sample cells, six references: seven waves -- eight needs six spilled registers with the tile: 12.1 against 9.8 ms per 341 4K16 chroma frame pairs,
// profiles/r6_degrain_tile_ab.txt)
template <int NR, int W> constexpr int dg_cell_waves() { return W <= 2 ? 7 : W == 4 ? (NR <= 4 ? 8 : NR <= 6 ? 7 : 6) : W == 8 ? (NR <= 2 ? 6 : NR <= 6 ? 5 : 4) : (NR <= 8 ? 3 : 2); }
template <typename T, int NR, int W>
__global__ __launch_bounds__(256, (dg_cell_waves<NR, W>())) void degrain_cell_kernel(const DGParams *Pp, const DGJob *jobs, const PlanRecT<NR> *plan, int planeFirst, int planesPerFrame) {
    typedef PlanRecT<NR> PlanRec;
    const DGParams &P = *Pp;
    const int bxi = blockIdx.x, byi = blockIdx.y, z = blockIdx.z;
    // (an XCD-contiguous tile order, measured r2 on 4K16 Degrain3, 512 frames: HBM fetch 124 -> 88 GB (luma) and 75 -> 34 GB (chroma), but the
    // launch gets 8 ms SLOWER -- 189 against 181 ms for everything but the search: the kernel is not HBM-bound)
    const int f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    const int c = bxi * 32 + (threadIdx.x & 31), y = byi * 8 + (threadIdx.x >> 5);
    const int x0 = c * W;
    // r6: the plan records of the blocks that cover this workgroup's tile (32 cells x 8 rows: with blocks overlapping by half 33 block columns x 2-5 block
    // rows) are fetched ONCE, cooperatively, into LDS.  Before, every thread read the records of its <= 4 covering blocks itself: three of the eleven memory
    // instructions of a block visit (12 of 45 per thread; a 16-byte load costs the texture addresser its 16 cycles whether or not the line is in L1), and each
    // visit was two dependent round trips (record -> reference rows)
    // Measured (profiles/r6_degrain_tile_ab.txt, ms per batch, every thread for itself -> tile): six 16-bit references 15.9 -> 14.3 (8-sample cells) and 12.8 -> 9.8
    // (4-sample cells), twelve 47.2 -> 43.0 / 29.2 -> 25.2; TWO 8-bit references (16-byte records, two loads per visit) lose: 15.5 -> 16.6, 12.7 -> 15.6 -- the tile is
    // for filters with six or more references (Degrain3-6)
    constexpr bool TILED = dg_tiled(NR);
    constexpr int RD = (int)sizeof(PlanRec) / 4;
    __shared__ __attribute__((aligned(16))) unsigned tileD[TILED ? DG_TILE_MAX * RD : 1];
    int tBx = 0, tBy = 0, tNbx = 0; // (wave-uniform: scalar registers)
    // (the window taps next to the tile -- the nine windows of 16x16 blocks are 4.5 KB -- measured and removed: 14.7 against 14.5 ms, cfg5's 8-sample cells 26.2 against 25.1:
    // profiles/r6_degrain_window_plan_ab.txt)
    if (TILED && g.process && P.overlap) { // (uniform over the workgroup; the host launches this kernel only when the tile fits: dg_tile_fits)
        const int xt = bxi * 32 * W, yt = byi * 8;
        tBx = __builtin_amdgcn_readfirstlane(BLK_FIRST(xt, g.blkW, g.stepX));
        tBy = __builtin_amdgcn_readfirstlane(BLK_FIRST(yt, g.blkH, g.stepY));
        const int bxHi = min(bxi * 32 + 31, P.nBlkX - 1), byHi = min((yt + 7) / g.stepY, P.nBlkY - 1);
        tNbx = __builtin_amdgcn_readfirstlane(bxHi - tBx + 1);
        const int nby = __builtin_amdgcn_readfirstlane(byHi - tBy + 1);
        if (tNbx > 0) {
            const unsigned *src = (const unsigned *)(plan + ((size_t)f * 2 + (p ? 1 : 0)) * P.nBlk);
            const int rowD = tNbx * RD;
            for (int r = 0; r < nby; r++) {
                DG_GL const unsigned *q = (DG_GL const unsigned *)dg_gl((const unsigned char *)(src + ((size_t)(tBy + r) * P.nBlkX + tBx) * RD));
                for (int k = threadIdx.x; k < rowD; k += 256) tileD[r * rowD + k] = q[k];
            }
        }
        __syncthreads();
    }
    if (x0 >= g.W || y >= g.H) return;
    const DGJob &J = jobs[f];
    const unsigned char *srow = J.src[p] + (long long)y * g.srcPitch + (long long)x0 * sizeof(T);
    unsigned char *drow = J.dst[p] + (long long)y * g.dstPitch + (long long)x0 * sizeof(T);
    const bool fullW = x0 + W <= g.W;
    int s[W];
    if (fullW) dg_load<T, W>(dg_gl(srow), s);
    else {
#pragma unroll
        for (int i = 0; i < W; i++) s[i] = x0 + i < g.W ? (int)((const T *)srow)[i] : 0;
    }
    int out[W];
#pragma unroll
    for (int i = 0; i < W; i++) out[i] = s[i];
    if (g.process && x0 < g.WB && y < g.HB && !P.overlap) {
        // r5: blocks side by side (MVDegrains.cpp:238-249: Degrain_C straight into the frame, no windows).  W divides the block width, so the cell lies in ONE
        // block: one plan record, one vector load per reference -- the per-sample gather this replaces took 42 of the 135 ms of a 2048-frame 1080p step
        const PlanRec &R = (plan + ((size_t)f * 2 + (p ? 1 : 0)) * P.nBlk)[(y / g.blkH) * P.nBlkX + x0 / g.blkW];
        const int px = x0 % g.blkW, py = y % g.blkH;
        const unsigned char *safe = nullptr;
#pragma unroll
        for (int r = 0; r < NR; r++) if (J.refs[r][p]) safe = J.refs[r][p];
        const long long rowOff = safe ? (long long)py * g.supPitch + (long long)px * sizeof(T) : 0;
        DgRaw<T, W> raw[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) raw[r] = dg_load_raw<T, W>(dg_gl((J.refs[r][p] ? J.refs[r][p] : (safe ? safe : J.src[p])) + R.off[r] + rowOff)); // (weight 0: any valid address)
        const int wsrc = R.wsrc, pm = (1 << P.bits) - 1;
        int sum[W];
#pragma unroll
        for (int i = 0; i < W; i++) sum[i] = 128 + s[i] * wsrc;
        dg_mad_refs<T, NR, W>(raw, R, sum);
#pragma unroll
        for (int i = 0; i < W; i++) {
            int o = (T)(sum[i] >> 8);
            if (g.limit < pm) { // MVDegrains.h:163-181
                const int lo = s[i] - g.limit, hi = s[i] + g.limit;
                o = o < lo ? lo : o;
                o = o > hi ? hi : o;
            }
            out[i] = o;
        }
    } else if (g.process && x0 < g.WB && y < g.HB) { // MVDegrains.cpp:211-214,238-249,290-298: uncovered strips keep the source
        const PlanRec *pl = plan + ((size_t)f * 2 + (p ? 1 : 0)) * P.nBlk;
        int bx1 = c; if (bx1 > P.nBlkX - 1) bx1 = P.nBlkX - 1; // (the step is the cell: no division)
        const int bx0 = BLK_FIRST(x0, g.blkW, g.stepX);
        int by0, by1;
        blk_cover(y, g.blkH, g.stepY, P.nBlkY, by0, by1);
        unsigned acc[W];
#pragma unroll
        for (int i = 0; i < W; i++) acc[i] = 0;
        const int16_t *win = P.win[p];
        // a frame outside the clip has no super frame: its loads (weight 0, plan offset 0) go to a super plane the job does have, so that
        // the row offset (super pitch) stays inside the buffer; a job without any reference reads the source plane at offset 0
        const unsigned char *refp[NR], *safe = nullptr;
#pragma unroll
        for (int r = 0; r < NR; r++) if (J.refs[r][p]) safe = J.refs[r][p];
#pragma unroll
        for (int r = 0; r < NR; r++) refp[r] = J.refs[r][p] ? J.refs[r][p] : (safe ? safe : J.src[p]);
        for (int by = by0; by <= by1; by++) {
            const int py = y - by * g.stepY;
            const int wby = BLK_WIN_ROW(by, P.nBlkY);
            for (int bx = bx0; bx <= bx1; bx++) {
                const int px = x0 - bx * g.stepX;   // >= 0; the block covers samples i < blkW - px of this cell
                const int nv = g.blkW - px;
                if (nv <= 0) continue;
                const int wbx = BLK_WIN_COL(bx, P.nBlkX);
                PlanRec R;
                if (TILED) __builtin_memcpy(&R, &tileD[((by - tBy) * tNbx + (bx - tBx)) * RD], sizeof(PlanRec));
                else R = pl[by * P.nBlkX + bx];
                const int wsrc = R.wsrc;
                int sum[W];
#pragma unroll
                for (int i = 0; i < W; i++) sum[i] = 128 + s[i] * wsrc;
                const long long rowOff = safe ? (long long)py * g.supPitch + (long long)px * sizeof(T) : 0;
                const int16_t *wrow = win + (wby + wbx) * g.blkW * g.blkH + py * g.blkW + px;
                DgRaw<unsigned short, W> wr; // the window taps of this row of the cell, packed (unpacked where they are used: four registers fewer across the weighted sums)
                if (nv >= W) { // whole cell inside the block: vector loads, ALL of the block's references requested before the first is used
                    // (a reference with weight 0 is loaded too -- from a valid address: refp -- which costs bandwidth the kernel has to
                    // spare; waiting for every load in turn, as a `if (w)` around each one makes the compiler do, cost 4x the round trips)
                    DgRaw<T, W> raw[NR];
#pragma unroll
                    for (int r = 0; r < NR; r++) raw[r] = dg_load_raw<T, W>(dg_gl(refp[r] + R.off[r] + rowOff));
                    wr = dg_load_raw<unsigned short, W>(dg_gl((const unsigned char *)wrow));
                    dg_mad_refs<T, NR, W>(raw, R, sum);
                } else { // partially covered (overlap != block/2): per-sample loads of the covered samples only
#pragma unroll
                    for (int r = 0; r < NR; r++) {
                        const int w = R.w[r];
                        if (w) {
                            const T *q = (const T *)(J.refs[r][p] + R.off[r] + rowOff);
#pragma unroll
                            for (int i = 0; i < W; i++) if (i < nv) sum[i] += (int)q[i] * w;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < (W + 1) / 2; k++) wr.d[k] = 0;
#pragma unroll
                    for (int i = 0; i < W; i++) if (i < nv) wr.d[i >> 1] |= (unsigned)(unsigned short)wrow[i] << (16 * (i & 1));
                }
#pragma unroll
                for (int i = 0; i < W; i++) {
                    const int val = (T)(sum[i] >> 8);
                    if (i < nv) acc[i] += (unsigned)((val * dg_sample<unsigned short, W>(wr, i)) >> 6);
                }
            }
        }
        const int pm = (1 << P.bits) - 1;
#pragma unroll
        for (int i = 0; i < W; i++) {
            if (x0 + i < g.WB) {
                unsigned a0 = acc[i];
                if (sizeof(T) == 1) a0 &= 0xffffu; // 16-bit accumulator of the 8-bit path (Overlap.cpp:254-256)
                const int a = (int)((a0 + 16) >> 5); // Overlap.cpp:335-356
                int o = a > pm ? pm : a;
                if (g.limit < pm) { // MVDegrains.h:163-181
                    const int lo = s[i] - g.limit, hi = s[i] + g.limit;
                    o = o < lo ? lo : o;
                    o = o > hi ? hi : o;
                }
                out[i] = o;
            }
        }
    }
    if (fullW) dg_store<T, W>(dg_glw(drow), out);
    else {
#pragma unroll
        for (int i = 0; i < W; i++) if (x0 + i < g.W) ((T *)drow)[i] = (T)out[i];
    }
}

// ------------------------------------------------------------------------------------------------ host objects

struct mvx_degrain {
    CallGuard guard;
    DGParams P;
    DevBuf<DGParams> dP;
    DevBuf<DGJob> dJobs;          // these two grow to twice the call's jobs
    DevBuf<int> dUsable;
    DevBuf<unsigned char> dPlan;  // grows to one and a half times the call's plan
    BlkWin win;
    int radius;
};

static int ensure_jobs(mvx_degrain *h, int nframes, size_t planBytesPerFrame) {
    const size_t n = (size_t)nframes, need = planBytesPerFrame * n;
    HIP_CHECK(h->dJobs.reserve(n, n));
    HIP_CHECK(h->dUsable.reserve(n * 12, n * 12));
    HIP_CHECK(h->dPlan.reserve(need, need / 2));
    return MVX_OK;
}

// MVDegrains.cpp:511-809 mvdegrainCreate
extern "C" __attribute__((visibility("default"))) int mvx_degrain_create(const mvx_degrain_args *a, const mvx_analysis_data *ad, const mvx_super *sup, const ptrdiff_t src_pitch[3],
                                  const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3], mvx_degrain **out, char *err) {
    MVX_CREATE_BEGIN(out);
    MVX_REFUSE_FLOAT(sup, "Degrain");
    const mvx_super_info &si = sup->info;
    const int radius = a->radius;
    if (radius < 1 || radius > 6) MVX_FAIL("Degrain: radius must be between 1 and 6.");
    char name[16]; // the reference's filter name carries the radius
    snprintf(name, sizeof(name), "Degrain%d", radius);
    mvx_degrain_n_args an; // (DegrainN without far thresholds: dg_resolve)
    an.radius = radius; an.thsad = a->thsad; an.thsadc = a->thsadc; an.thsad2 = an.thsadc2 = MVX_UNSET;
    an.plane = a->plane; an.limit = a->limit; an.limitc = a->limitc; an.thscd1 = a->thscd1; an.thscd2 = a->thscd2;
    DgResolved r;
    if (int rc = dg_resolve(name, &an, DG_PLAIN, ad, si, &r, err)) return rc;
    mvx_degrain *h;
    if (int rc = blk_new(&h, ad, si, src_pitch, super_pitch, dst_pitch, err)) return rc;
    h->radius = radius;
    DGParams &P = h->P;
    P.nRefs = 2 * radius;
    P.thSAD[0] = r.info.thsad_d[0]; P.thSAD[1] = r.info.thsadc_d[0];
    dg_apply(P, r, si);
    *out = h;
    return MVX_OK;
}

extern "C" __attribute__((visibility("default"))) void mvx_degrain_destroy(mvx_degrain *d) { delete d; }

// The caller promises that every reference super frame of every job carries, behind its luma plane at + copy_stride[0], the plane shifted left by
// one sample (mvx_super_shadow_frames).  Only changes which addresses the kernels load from.
extern "C" __attribute__((visibility("default"))) int mvx_degrain_set_ref_shadow(mvx_degrain *d, const ptrdiff_t copy_stride[3]) {
    const long long v = copy_stride ? (long long)copy_stride[0] : 0;
    const PlaneG &g0 = d->P.pl[0];
    if (v < 0 || v % 16) { mvx_set_error("mvx_degrain_set_ref_shadow: copy strides must be non-negative multiples of 16 bytes"); return MVX_E_ARG; }
    // (plan records hold 32-bit byte offsets into a super plane: the copy must lie inside that range)
    if (v && v + g0.supPlaneStride * d->P.pel * d->P.pel >= 0xffffffffLL) { mvx_set_error("mvx_degrain_set_ref_shadow: the shifted copy lies beyond 4 GiB of the plane"); return MVX_E_ARG; }
    std::lock_guard<std::mutex> lk(d->guard.mu);
    d->P.pl[0].shadow = d->P.bps == 2 ? v : 0;
    if (d->dP.p) HIP_CHECK(hipMemcpy(d->dP.p, &d->P, sizeof(DGParams), hipMemcpyHostToDevice));
    return MVX_OK;
}

template <typename T> static void launch_degrain(int nr, dim3 grid, hipStream_t st, const DGParams *dP, const DGJob *dJ, const void *plan) {
#define DG(N) hipLaunchKernelGGL((degrain_kernel<T, N>), grid, dim3(256), 0, st, dP, dJ, (const PlanRecT<N> *)plan)
    switch (nr) { case 2: DG(2); break; case 4: DG(4); break; case 6: DG(6); break; case 8: DG(8); break; case 10: DG(10); break; default: DG(12); break; }
#undef DG
}

template <typename T, int W> static void launch_degrain_cells_w(int nr, dim3 grid, hipStream_t st, const DGParams *dP, const DGJob *dJ, const void *plan, int p0, int npl) {
#define DGC(N) hipLaunchKernelGGL((degrain_cell_kernel<T, N, W>), grid, dim3(256), 0, st, dP, dJ, (const PlanRecT<N> *)plan, p0, npl)
    switch (nr) { case 2: DGC(2); break; case 4: DGC(4); break; case 6: DGC(6); break; case 8: DGC(8); break; case 10: DGC(10); break; default: DGC(12); break; }
#undef DGC
}
template <typename T> static void launch_degrain_cells(int nr, int W, dim3 grid, hipStream_t st, const DGParams *dP, const DGJob *dJ, const void *plan, int p0, int npl) {
    switch (W) {
    case 2: launch_degrain_cells_w<T, 2>(nr, grid, st, dP, dJ, plan, p0, npl); break;
    case 4: launch_degrain_cells_w<T, 4>(nr, grid, st, dP, dJ, plan, p0, npl); break;
    case 8: launch_degrain_cells_w<T, 8>(nr, grid, st, dP, dJ, plan, p0, npl); break;
    default: launch_degrain_cells_w<T, 16>(nr, grid, st, dP, dJ, plan, p0, npl); break;
    }
}

extern "C" __attribute__((visibility("default"))) int mvx_degrain_frames(mvx_degrain *d, int nframes, const mvx_degrain_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    const DGParams &P = d->P;
    for (int f = 0; f < nframes; f++) {
        if (int rc = fps_check_planes("mvx_degrain_frames", "src", jobs[f].src, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_degrain_frames", "dst", jobs[f].dst, P.nplanes, P.bps, true)) return rc;
        for (int r = 0; r < P.nRefs; r++)
            if (int rc = fps_check_planes("mvx_degrain_frames", "reference super", jobs[f].refs[r], P.nplanes, 16, false)) return rc;
    }
    CallGuard::Scope scope(d->guard, st);
    int rc = blk_upload(d->dP, d->P, d->win);
    if (rc) return rc;
    if ((rc = ensure_jobs(d, nframes, plan_rec_bytes(P.nRefs) * 2 * (size_t)P.nBlk))) return rc;
    std::vector<DGJob> hj(nframes);
    for (int f = 0; f < nframes; f++) {
        memset(&hj[f], 0, sizeof(DGJob));
        for (int p = 0; p < 3; p++) { hj[f].src[p] = (const unsigned char *)jobs[f].src[p]; hj[f].dst[p] = (unsigned char *)jobs[f].dst[p]; }
        for (int r = 0; r < P.nRefs; r++) {
            for (int p = 0; p < 3; p++) hj[f].refs[r][p] = (const unsigned char *)jobs[f].refs[r][p];
            hj[f].blobs[r] = (const unsigned char *)jobs[f].blobs[r];
        }
    }
    HIP_CHECK(hipMemcpyAsync(d->dJobs.p, hj.data(), sizeof(DGJob) * nframes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(usable_kernel, dim3(P.nRefs, nframes), dim3(256), 0, st, d->dP.p, d->dJobs.p, d->dUsable.p);
    {
        const dim3 pg((P.nBlk + 255) / 256, nframes);
#define DGP(N) hipLaunchKernelGGL(degrain_plan_kernel<N>, pg, dim3(256), 0, st, d->dP.p, d->dJobs.p, d->dUsable.p, (PlanRecT<N> *)d->dPlan.p)
        switch (P.nRefs) { case 2: DGP(2); break; case 4: DGP(4); break; case 6: DGP(6); break; case 8: DGP(8); break; case 10: DGP(10); break; default: DGP(12); break; }
#undef DGP
    }
    // overlapped blocks with a power-of-two step: vectorised cell kernel, one launch per plane class; otherwise the
    // per-sample gather
    // (r5: blocks side by side take the cell kernel too -- a cell of 8 (4) samples inside one block)
    auto cellW = [&](int p) { const int w = P.pl[p].stepX; return P.overlap ? ((w == 2 || w == 4 || w == 8 || w == 16) ? w : 0) : (P.pl[p].blkW % 8 == 0 ? 8 : P.pl[p].blkW % 4 == 0 ? 4 : 0); };
    auto tileOk = [&](int p) { return !dg_tiled(P.nRefs) || !P.overlap || dg_tile_fits(P.pl[p].blkW, P.pl[p].blkH, P.pl[p].stepX, P.pl[p].stepY); };
    const bool cells = cellW(0) && tileOk(0) && (P.nplanes == 1 || (cellW(1) && P.pl[1].stepX == P.pl[2].stepX && tileOk(1) && tileOk(2)));
    if (cells) {
        for (int cls = 0; cls < (P.nplanes > 1 ? 2 : 1); cls++) {
            const int p0 = cls, npl = cls ? 2 : 1, W = cellW(p0);
            dim3 grid(((P.pl[p0].W + W - 1) / W + 31) / 32, (P.pl[p0].H + 7) / 8, nframes * npl);
            if (P.bps == 1) launch_degrain_cells<uint8_t>(P.nRefs, W, grid, st, d->dP.p, d->dJobs.p, d->dPlan.p, p0, npl);
            else launch_degrain_cells<uint16_t>(P.nRefs, W, grid, st, d->dP.p, d->dJobs.p, d->dPlan.p, p0, npl);
        }
    } else {
        dim3 grid((P.pl[0].W + 63) / 64, (P.pl[0].H + 3) / 4, nframes * 3);
        if (P.bps == 1) launch_degrain<uint8_t>(P.nRefs, grid, st, d->dP.p, d->dJobs.p, d->dPlan.p);
        else launch_degrain<uint16_t>(P.nRefs, grid, st, d->dP.p, d->dJobs.p, d->dPlan.p);
    }
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}

// ================================================================================================ mv.SCDetection
// MVSCDetection.c:43-73: _SceneChangePrev / _SceneChangeNext = !fgopIsUsable(vectors at n) (Fakery.c:52-58,144-146)
__global__ __launch_bounds__(256) void scdetect_kernel(const unsigned char *const *blobs, int nLvCount, int nBlk, long long thscd1, int thscd2, int *out) {
    const bool ok = fps_block_usable(blobs[blockIdx.x], true, nLvCount, nBlk, thscd1, thscd2);
    if (threadIdx.x == 0) out[blockIdx.x] = !ok;
}

extern "C" __attribute__((visibility("default"))) int mvx_scdetect(const mvx_analysis_data *ad, int64_t thscd1, int32_t thscd2, int n, const void *const *blobs,
                                                                   int32_t *scene_change, void *stream, char *err) {
    MVX_ERR_BEGIN();
    if (n <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    int64_t s1; int32_t s2;
    if (int rc = mvx_resolve_thscd("SCDetection", thscd1, thscd2, ad, &s1, &s2, err)) return rc;
    DevBuf<const unsigned char *> dB; // (freed on return, after the stream has been waited for)
    DevBuf<int> dOut;
    HIP_CHECK(dB.reserve(n));
    if (dOut.reserve(n) != hipSuccess) { mvx_set_error("mvx_scdetect: out of device memory"); return MVX_E_NOMEM; }
    hipError_t e = hipMemcpyAsync(dB.p, blobs, sizeof(void *) * n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(scdetect_kernel, dim3(n), dim3(256), 0, st, dB.p, ad->nLvCount, ad->nBlkX * ad->nBlkY, (long long)s1, (int)s2, dOut.p);
        e = hipMemcpyAsync(scene_change, dOut.p, sizeof(int) * n, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { mvx_set_error("mvx_scdetect: %s", hipGetErrorString(e)); return MVX_E_DEVICE; }
    return MVX_OK;
}
