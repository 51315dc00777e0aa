// mvx_degrain.hip -- the block filters on gfx950: mv.Degrain1..6 (first half), mv.BlockFPS and mv.SCDetection (second half, each under its own
// heading).  What they share with DegrainN, Compensate and CompensateN (mvx_degrain_n.hip, mvx_compensate.hip) is in mvx_block_shared.h, what
// they share with the flow filters and mv.Mask in mvx_fps_shared.h.
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

struct DGCommon {
    CallGuard guard;
    DGParams P;
    DevBuf<DGParams> dP;
    DevBuf<DGJob> dJobs;          // these two grow to twice the call's jobs
    DevBuf<int> dUsable;
    DevBuf<unsigned char> dPlan;  // grows to one and a half times the call's plan
    BlkWin win;
};
struct mvx_degrain : DGCommon { int radius; };

static int ensure_jobs(DGCommon *h, int nframes, size_t planBytesPerFrame) {
    const size_t n = (size_t)nframes, need = planBytesPerFrame * n;
    HIP_CHECK(h->dJobs.reserve(n, n));
    HIP_CHECK(h->dUsable.reserve(n * 12, n * 12));
    HIP_CHECK(h->dPlan.reserve(need, need / 2));
    return MVX_OK;
}

// samples per thread of BlockFPS's row kernel: up to 16 bytes, dividing the block width and the frame width, so that a segment is never split
// between cases (the uncovered strip starts at nBlkX * blkW).  0: the blocks overlap or are not powers of two -- the per-sample gather
static int dg_rows_cw(const DGParams &P, int p) {
    if (P.overlap) return 0;
    const PlaneG &g = P.pl[p];
    int cw = 16 / P.bps;
    while (cw > 1 && (g.blkW % cw || g.W % cw)) cw >>= 1;
    return (cw >= 2 && (g.blkW & (g.blkW - 1)) == 0 && (g.blkH & (g.blkH - 1)) == 0) ? cw : 0;
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

// ================================================================================================ mv.BlockFPS
// MVBlockFPS.c:229-676 (frame), :741-1014 (creation); MaskFun.cpp:63-166,349-371; SimpleResize.cpp:27-121.
// One gather pass per output sample like Degrain / Compensate: the two motion-compensated fetches (backward vectors at
// the left frame into the right super frame, forward vectors at the right frame into the left one, both scaled by the
// time position), the per-mode blend, the overlap window sum and ToPixels.  The occlusion / SAD masks live at block
// resolution (three small byte planes per frame pair) and are upsized bilinearly ON THE FLY per sample with the
// reference's integer tables, so no full-size mask planes exist.

struct BFParams {
    int mode, blend, XP, YP;            // padded small-mask grid
    int nWidthP[2], nHeightP[2];        // luma / chroma upsizer output sizes
    double ml;
    long long thscd1; int thscd2;
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
__global__ __launch_bounds__(256) void bf_usable_kernel(const DGParams *Pp, const BFParams *Bp, const BFJob *jobs, int *usable) {
    const DGParams &P = *Pp; const BFParams &B = *Bp;
    const BFJob &J = jobs[blockIdx.x];
    const unsigned char *const blobs[2] = { J.blobF, J.blobB };
    const bool ok = fps_block_usable(blobs, J.good && J.time256 > 0 && J.time256 < 256, P.nLvCount, P.nBlk, B.thscd1, B.thscd2);
    if (threadIdx.x == 0) usable[blockIdx.x] = ok;
}

// small masks, pass 1: scatter-max (occlusion, MaskFun.cpp:91-130) or direct (SAD mask, :139-166) into int planes
// [job][F,B][YP*XP]; the scatter only ever takes maxima, so the order of the reference's loops does not matter.
__global__ __launch_bounds__(256) void bf_mask_kernel(const DGParams *Pp, const BFParams *Bp, const BFJob *jobs, const int *usable, int *small) {
    const DGParams &P = *Pp; const BFParams &B = *Bp;
    const int f = blockIdx.z, dir = blockIdx.y; // dir 0 = forward mask, 1 = backward mask
    if (!usable[f] || B.mode < 3) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.nBlk) return;
    const BFJob &J = jobs[f];
    const GVecD *vec = mvx_level0((dir ? J.blobB : J.blobF), P.nLvCount);
    const int nBlkX = P.nBlkX, nBlkY = P.nBlkY, by = i / nBlkX, bx = i - by * nBlkX;
    const int time256 = dir ? 256 - J.time256 : J.time256;
    const int stepX = P.pl[0].stepX, stepY = P.pl[0].stepY, nPel = P.pel;
    int *m = small + ((size_t)f * 2 + dir) * B.XP * B.YP;
    if (B.mode <= 5) {
        fps_occlusion_block(vec, i, bx, by, nBlkX, nBlkY, dir, time256, stepX, stepY, nPel, B.ml, m, B.XP);
    } else {
        const int tX = (256 - time256) * 16 / (stepX * nPel), tY = (256 - time256) * 16 / (stepY * nPel);
        int bxi = bx - vec[i].x * tX / 4096, byi = by - vec[i].y * tY / 4096;
        if (bxi < 0 || bxi >= nBlkX || byi < 0 || byi >= nBlkY) { bxi = bx; byi = by; }
        const long long sad = vec[bxi + byi * nBlkX].sad >> (P.bits - 8);
        const double factor = 4.0 / (B.ml * P.pl[0].blkW * P.pl[0].blkH);
        const double l = 255 * ((double)sad * factor); // pow(x, 1.0) == x
        m[bx + by * B.XP] = (int)(unsigned char)((l > 255) ? 255 : l);
    }
}
// pass 2: byte planes [job][F,B,O][YP*XP] with the right / bottom padding clones (MaskFun.cpp:63-80) and O = F*B/255 (:93-101)
__global__ __launch_bounds__(256) void bf_mask_finish_kernel(const DGParams *Pp, const BFParams *Bp, const int *usable, const int *small, unsigned char *masks) {
    const DGParams &P = *Pp; const BFParams &B = *Bp;
    const int f = blockIdx.y;
    if (!usable[f] || B.mode < 3) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B.XP * B.YP) return;
    const int y = i / B.XP, x = i - y * B.XP;
    const int s = fps_pad_source(x, y, P.nBlkX, P.nBlkY, B.XP);
    const int *mF = small + ((size_t)f * 2 + 0) * B.XP * B.YP, *mB = small + ((size_t)f * 2 + 1) * B.XP * B.YP;
    const int vF = mF[s], vB = mB[s];
    unsigned char *o = masks + (size_t)f * 3 * B.XP * B.YP;
    o[i] = (unsigned char)vF;
    o[B.XP * B.YP + i] = (unsigned char)vB;
    o[2 * B.XP * B.YP + i] = (unsigned char)((vF * vB) / 255);
}

__global__ __launch_bounds__(256) void bf_plan_kernel(const DGParams *Pp, const BFJob *jobs, const int *usable, BFPlan *plan) {
    const DGParams &P = *Pp;
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

__device__ __forceinline__ int bf_median(int a, int b, int c) { const int mn = min(a, b), mx = max(a, b); return max(mn, min(mx, c)); }

template <typename T>
__global__ __launch_bounds__(256) void blockfps_kernel(const DGParams *Pp, const BFParams *Bp, const BFJob *jobs, const int *usable, const BFPlan *plan, const unsigned char *masks) {
    const DGParams &P = *Pp; const BFParams &B = *Bp;
    const int z = blockIdx.z, f = z / 3, p = z % 3;
    if (p >= P.nplanes) return;
    const PlaneG &g = P.pl[p];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const BFJob &J = jobs[f];
    T *drow = (T *)(J.dst[p] + (long long)y * g.dstPitch);
    const int t = J.time256;
    if (!usable[f]) { // time256 0 / 256, vectors unusable or frames outside the clip (:285-288, :640-673)
        const int l = ((const T *)(J.clipL[p] + (long long)y * B.clipPitch[p]))[x];
        if (t <= 0 || (t < 256 && !B.blend)) { drow[x] = (T)l; return; }
        const int r = ((const T *)(J.clipR[p] + (long long)y * B.clipPitch[p]))[x];
        drow[x] = t >= 256 ? (T)r : (T)((l * (256 - t) + r * t) >> 8);
        return;
    }
    const int sVal = ((const T *)(J.srcSup[p] + B.supInterior[p] + (long long)y * g.supPitch))[x];
    const int rVal = ((const T *)(J.refSup[p] + B.supInterior[p] + (long long)y * g.supPitch))[x];
    const int covW = P.overlap ? g.WB : g.blkW * P.nBlkX, covH = P.overlap ? g.HB : g.blkH * P.nBlkY;
    if (x >= covW || y >= covH) { drow[x] = (T)((sVal * (256 - t) + rVal * t) >> 8); return; } // Blend of the uncovered strips
    const int mode = B.mode, c = p ? 1 : 0;
    int mF = 0, mB = 0, mO = 0;
    if (mode >= 3) {
        const unsigned char *m = masks + (size_t)f * 3 * B.XP * B.YP;
        if (mode != 5 && mode != 8) {
            mF = bf_upsize(m, B.XP, B.hOff[c], B.hW[c], B.vOff[c], B.vW[c], x, y);
            mB = bf_upsize(m + B.XP * B.YP, B.XP, B.hOff[c], B.hW[c], B.vOff[c], B.vW[c], x, y);
        }
        if (mode == 4 || mode == 5 || mode == 7 || mode == 8) mO = bf_upsize(m + 2 * B.XP * B.YP, B.XP, B.hOff[c], B.hW[c], B.vOff[c], B.vW[c], x, y);
    }
    const BFPlan *pl = plan + (size_t)f * P.nBlk;
    auto result = [&](const BFPlan &R, int px, int py) -> int { // RealResultBlock, MVBlockFPS.c:117-227
        const int b = ((const T *)(J.refSup[p] + R.offB[c] + (long long)py * g.supPitch))[px];
        const int fw = ((const T *)(J.srcSup[p] + R.offF[c] + (long long)py * g.supPitch))[px];
        switch (mode) {
        case 0: return (b * t + fw * (256 - t)) >> 8;
        case 1: return bf_median(rVal, sVal, (int)(T)((b * t + fw * (256 - t)) >> 8));
        case 2: return bf_median((int)(T)((rVal * t + sVal * (256 - t)) >> 8), b, fw);
        case 3: case 6: return (((mB * fw + (255 - mB) * b + 255) >> 8) * t + ((mF * b + (255 - mF) * fw + 255) >> 8) * (256 - t)) >> 8;
        case 4: case 7: {
            const int ff = (mF * b + (255 - mF) * fw + 255) >> 8, bb = (mB * fw + (255 - mB) * b + 255) >> 8;
            const int avg = (rVal * t + sVal * (256 - t) + 255) >> 8, m = (bb * t + ff * (256 - t)) >> 8;
            return (avg * mO + m * (255 - mO) + 255) >> 8;
        }
        default: return mO << (P.bits - 8);
        }
    };
    int out;
    if (!P.overlap) {
        const int bx = x / g.blkW, by = y / g.blkH;
        out = (T)result(pl[by * P.nBlkX + bx], x - bx * g.blkW, y - by * g.blkH);
    } else {
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
                const int val = (T)result(pl[by * P.nBlkX + bx], px, py);
                acc += (unsigned)((val * (int)win[(wby + wbx) * g.blkW * g.blkH + py * g.blkW + px]) >> 6);
            }
        }
        if (sizeof(T) == 1) acc &= 0xffffu;
        const int a = (int)((acc + 16) >> 5);
        const int pm = (1 << P.bits) - 1;
        out = a > pm ? pm : a;
    }
    drow[x] = (T)out;
}


// ---- blocks without overlap: one thread per CW consecutive samples of one block row (the host checks dg_rows_cw's conditions).
// The four vector loads (left / right frame at the sample, the two motion-compensated fetches) and the plan record are per segment;
// the mask upsizer (SimpleResize.cpp:62-121) interpolates vertically once per mask column the segment touches.
template <typename T, int CW>
__global__ __launch_bounds__(256) void blockfps_rows_kernel(const DGParams *Pp, const BFParams *Bp, const BFJob *jobs, const int *usable, const BFPlan *plan, const unsigned char *masks,
                                                            int planeFirst, int planesPerFrame) {
    const DGParams &P = *Pp; const BFParams &B = *Bp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * CW, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const BFJob &J = jobs[f];
    unsigned char *dptr = J.dst[p] + (long long)y * g.dstPitch + (long long)x * (long long)sizeof(T);
    const int t = J.time256;
    int out[CW];
    if (!usable[f]) { // time256 0 / 256, vectors unusable or frames outside the clip (:285-288, :640-673)
        int l[CW];
        dg_load<T, CW>(dg_gl(J.clipL[p] + (long long)y * B.clipPitch[p] + (long long)x * (long long)sizeof(T)), l);
        if (t <= 0 || (t < 256 && !B.blend)) { dg_store<T, CW>(dg_glw(dptr), l); return; }
        int r[CW];
        dg_load<T, CW>(dg_gl(J.clipR[p] + (long long)y * B.clipPitch[p] + (long long)x * (long long)sizeof(T)), r);
#pragma unroll
        for (int i = 0; i < CW; i++) out[i] = t >= 256 ? r[i] : (int)(T)((l[i] * (256 - t) + r[i] * t) >> 8);
        dg_store<T, CW>(dg_glw(dptr), out);
        return;
    }
    int sVal[CW], rVal[CW];
    const long long inner = B.supInterior[p] + (long long)y * g.supPitch + (long long)x * (long long)sizeof(T);
    dg_load<T, CW>(dg_gl(J.srcSup[p] + inner), sVal);
    dg_load<T, CW>(dg_gl(J.refSup[p] + inner), rVal);
    const int covW = g.blkW * P.nBlkX, covH = g.blkH * P.nBlkY;
    if (x >= covW || y >= covH) { // Blend of the uncovered strips
#pragma unroll
        for (int i = 0; i < CW; i++) out[i] = (int)(T)((sVal[i] * (256 - t) + rVal[i] * t) >> 8);
        dg_store<T, CW>(dg_glw(dptr), out);
        return;
    }
    const int mode = B.mode, c = p ? 1 : 0;
    int mF[CW], mB[CW], mO[CW];
#pragma unroll
    for (int i = 0; i < CW; i++) { mF[i] = 0; mB[i] = 0; mO[i] = 0; }
    if (mode >= 3) {
        DG_GL const unsigned char *m = dg_gl(masks + (size_t)f * 3 * B.XP * B.YP);
        // (r4: the resize tables and the mask bytes through global-address-space pointers and as vectors -- the table pointers sit in a struct, so the
        // compiler emitted one FLAT load per table entry, each waited for on its own, and six byte loads per mask: 45 loads per thread, now 15)
        const int wb = *(DG_GL const int *)dg_gl(B.vW[c] + y), wt = 16384 - wb;
        const int rowOff = *(DG_GL const int *)dg_gl(B.vOff[c] + y) * B.XP;
        int hO[CW], hWr[CW];
        if (x + CW <= g.W) {
            dg_load_ints<CW>(dg_gl(B.hOff[c] + x), hO);
            dg_load_ints<CW>(dg_gl(B.hW[c] + x), hWr);
        } else {
#pragma unroll
            for (int i = 0; i < CW; i++) { const int xi = x + i < g.W ? x + i : g.W - 1; hO[i] = *(DG_GL const int *)dg_gl(B.hOff[c] + xi); hWr[i] = *(DG_GL const int *)dg_gl(B.hW[c] + xi); }
        }
        const int o0 = hO[0];
        // vertically interpolated values of up to three mask columns; columns further right (upsizing by less than CW) are done on demand
        auto vcol = [&](DG_GL const unsigned char *mm, int o) { return (int)(unsigned char)((mm[rowOff + o] * wt + mm[rowOff + B.XP + o] * wb + 8192) >> 14); };
        auto upsize = [&](DG_GL const unsigned char *mm, int *dst) {
            // (the third column is only used when a sample's left neighbour is o0 + 1; at the plane's right edge it does not exist: read o0 + 1 again)
            // the bytes o0 .. o0 + 3 of the two mask rows as ONE unaligned dword each (the mask buffer has four bytes of slack behind its last row)
            const unsigned r0 = *(DG_GL const dg_uv1 *)(mm + rowOff + o0), r1 = *(DG_GL const dg_uv1 *)(mm + rowOff + B.XP + o0);
            auto vc = [&](int k) { return (int)(unsigned char)((((r0 >> (8 * k)) & 0xffu) * wt + ((r1 >> (8 * k)) & 0xffu) * wb + 8192) >> 14); };
            const int a0 = vc(0), a1 = vc(1), a2 = o0 + 2 < B.XP ? vc(2) : a1;
#pragma unroll
            for (int i = 0; i < CW; i++) {
                const int o = hO[i], wr = hWr[i], wl = 16384 - wr, k = o - o0;
                int a, b;
                if (k == 0) { a = a0; b = a1; } else if (k == 1) { a = a1; b = a2; } else { a = vcol(mm, o); b = vcol(mm, o + 1); }
                dst[i] = (int)(unsigned char)((a * wl + b * wr + 8192) >> 14);
            }
        };
        if (mode != 5 && mode != 8) { upsize(m, mF); upsize(m + B.XP * B.YP, mB); }
        if (mode == 4 || mode == 5 || mode == 7 || mode == 8) upsize(m + 2 * B.XP * B.YP, mO);
    }
    const int lbw = __ffs(g.blkW) - 1, lbh = __ffs(g.blkH) - 1;
    const int bx = x >> lbw, by = y >> lbh, px = x & (g.blkW - 1), py = y & (g.blkH - 1);
    const BFPlan R = plan[(size_t)f * P.nBlk + by * P.nBlkX + bx];
    int bv[CW], fv[CW];
    const long long bo = (long long)py * g.supPitch + (long long)px * (long long)sizeof(T);
    dg_load<T, CW>(dg_gl(J.refSup[p] + R.offB[c] + bo), bv);
    dg_load<T, CW>(dg_gl(J.srcSup[p] + R.offF[c] + bo), fv);
#pragma unroll
    for (int i = 0; i < CW; i++) { // RealResultBlock, MVBlockFPS.c:117-227
        const int b = bv[i], fw = fv[i];
        int v;
        switch (mode) {
        case 0: v = (b * t + fw * (256 - t)) >> 8; break;
        case 1: v = bf_median(rVal[i], sVal[i], (int)(T)((b * t + fw * (256 - t)) >> 8)); break;
        case 2: v = bf_median((int)(T)((rVal[i] * t + sVal[i] * (256 - t)) >> 8), b, fw); break;
        case 3: case 6: v = (((mB[i] * fw + (255 - mB[i]) * b + 255) >> 8) * t + ((mF[i] * b + (255 - mF[i]) * fw + 255) >> 8) * (256 - t)) >> 8; break;
        case 4: case 7: {
            const int ff = (mF[i] * b + (255 - mF[i]) * fw + 255) >> 8, bb = (mB[i] * fw + (255 - mB[i]) * b + 255) >> 8;
            const int avg = (rVal[i] * t + sVal[i] * (256 - t) + 255) >> 8, mm = (bb * t + ff * (256 - t)) >> 8;
            v = (avg * mO[i] + mm * (255 - mO[i]) + 255) >> 8; break;
        }
        default: v = mO[i] << (P.bits - 8); break;
        }
        out[i] = (int)(T)v;
    }
    dg_store<T, CW>(dg_glw(dptr), out);
}

#include "mvx_blockfps_float_rule.h"

// ---- float clips (mvx_blockfps_create_float): one kernel of cn_cell_kernel<float, W>'s shape for every case.  A thread produces one row of a cell
// of W float32 samples; W divides the block width and the block step, so the same <= 2 x 2 blocks cover all of a cell and each costs one
// vector load per fetch.  The usable pass, the masks, the plan and the resize tables are those above (none of them touches a sample; the plan's
// offsets are in bytes of 4 per sample because P.bps is 4).  The arithmetic is mvx_blockfps_float_rule.h; the copies of an unusable job move
// bytes and never look at them.  Job, plane, geometry and tables are uniform over the workgroup and arrive through scalar loads.  The
// motion-compensated fetches are 4-byte aligned and no more, as are the clip and the output planes.
// n: the samples of the cell inside the plane (W or more: all of them); a cell cut by the plane's edge is read and written sample by sample
template <int W> __device__ __forceinline__ DgRaw<float, W> bff_load(DG_GL const unsigned char *p, int n) {
    if (n >= W) return dg_load_raw<float, W>(p);
    DgRaw<float, W> r;
#pragma unroll
    for (int i = 0; i < W; i++) r.d[i] = i < n ? *(DG_GL const dg_uv1 *)(p + 4 * i) : 0u;
    return r;
}
template <int W> __device__ __forceinline__ void bff_store(DG_GL unsigned char *p, const DgRaw<float, W> &r, int n) {
    if (n >= W) {
        if constexpr (W == 4) { dg_uv4 t = { r.d[0], r.d[1], r.d[2], r.d[3] }; *(DG_GL dg_uv4 *)p = t; }
        else if constexpr (W == 2) { dg_uv2 t = { r.d[0], r.d[1] }; *(DG_GL dg_uv2 *)p = t; }
        else *(DG_GL dg_uv1 *)p = r.d[0];
        return;
    }
#pragma unroll
    for (int i = 0; i < W; i++) if (i < n) *(DG_GL dg_uv1 *)(p + 4 * i) = r.d[i];
}

// MODE: 0..5, the arithmetic of the mode (6, 7 and 8 compute like 3, 4 and 5: they differ in how the masks are made).  A template argument so
// that a mode keeps in registers only what it reads: 0..2 no mask, 3 F and B, 4 all three, 5 O alone and no fetch.  The masks of a sample
// travel packed in one register: F | B << 8 | O << 16
// The mask modes divide two or three times per sample, and an IEEE division is a dozen instructions with half a dozen values in flight.  Left
// alone the scheduler interleaves the divisions of all W samples (109 and 112 VGPRs at W = 4 in modes 3 and 4, occupancy 4); a scheduling
// barrier after each sample keeps one sample's temporaries live at a time
#define BFF_ONE_AT_A_TIME() do { if constexpr (MODE == 3 || MODE == 4) __builtin_amdgcn_sched_barrier(0); } while (0)
template <int W, int MODE>
__global__ __launch_bounds__(256) void bf_cell_float_kernel(const DGParams *Pp, const BFParams *Bp, const BFJob *jobs, const int *usable, const BFPlan *plan, const unsigned char *masks,
                                                            int planeFirst, int planesPerFrame) {
    static_assert(W == 1 || W == 2 || W == 4, "cells of 16 bytes at most");
    const DGParams &P = *Pp; const BFParams &B = *Bp;
    const int z = blockIdx.z, f = z / planesPerFrame, p = planeFirst + z % planesPerFrame;
    const PlaneG &g = P.pl[p];
    const int x0 = (blockIdx.x * 32 + (threadIdx.x & 31)) * W, y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x0 >= g.W || y >= g.H) return;
    const int n = g.W - x0;
    const BFJob &J = jobs[f];
    DG_GL unsigned char *dptr = dg_glw(J.dst[p]) + (long long)y * g.dstPitch + (long long)x0 * 4;
    const int t = J.time256;
    DgRaw<float, W> out;
    if (!usable[f]) { // time256 0 / 256, vectors unusable or frames outside the clip: a copy, bit for bit, or the blend of the two clip frames
        const long long co = (long long)y * B.clipPitch[p] + (long long)x0 * 4;
        const bool left = t <= 0 || (t < 256 && !B.blend);
        if (left || t >= 256) { bff_store<W>(dptr, bff_load<W>(dg_gl(left ? J.clipL[p] : J.clipR[p]) + co, n), n); return; }
        const DgRaw<float, W> l = bff_load<W>(dg_gl(J.clipL[p]) + co, n), r = bff_load<W>(dg_gl(J.clipR[p]) + co, n);
#pragma unroll
        for (int i = 0; i < W; i++) out.d[i] = __float_as_uint(mvx_bff_time(__uint_as_float(r.d[i]), __uint_as_float(l.d[i]), t));
        bff_store<W>(dptr, out, n);
        return;
    }
    const long long inner = B.supInterior[p] + (long long)y * g.supPitch + (long long)x0 * 4;
    const DgRaw<float, W> sVal = bff_load<W>(dg_gl(J.srcSup[p]) + inner, n), rVal = bff_load<W>(dg_gl(J.refSup[p]) + inner, n);
    const int covW = P.overlap ? g.WB : g.blkW * P.nBlkX, covH = P.overlap ? g.HB : g.blkH * P.nBlkY;
    if (x0 >= covW || y >= covH) { // the strips no block covers
#pragma unroll
        for (int i = 0; i < W; i++) out.d[i] = __float_as_uint(mvx_bff_time(__uint_as_float(rVal.d[i]), __uint_as_float(sVal.d[i]), t));
        bff_store<W>(dptr, out, n);
        return;
    }
    // from here on the cell lies inside the covered width (a multiple of W), so inside the plane
    const int c = p ? 1 : 0;
    unsigned mk[W];
#pragma unroll
    for (int i = 0; i < W; i++) mk[i] = 0u;
    if constexpr (MODE >= 3) { // the upsizer of blockfps_rows_kernel: the integer tables, the masks stay bytes
        DG_GL const unsigned char *m = dg_gl(masks + (size_t)f * 3 * B.XP * B.YP);
        const int wb = *(DG_GL const int *)dg_gl(B.vW[c] + y), wt = 16384 - wb;
        const int rowOff = *(DG_GL const int *)dg_gl(B.vOff[c] + y) * B.XP;
        int hO[W], hWr[W];
        dg_load_ints<W>(dg_gl(B.hOff[c] + x0), hO);
        dg_load_ints<W>(dg_gl(B.hW[c] + x0), hWr);
        const int o0 = hO[0];
        auto vcol = [&](DG_GL const unsigned char *mm, int o) { return (int)(unsigned char)((mm[rowOff + o] * wt + mm[rowOff + B.XP + o] * wb + 8192) >> 14); };
        auto upsize = [&](DG_GL const unsigned char *mm, int shift) {
            // the bytes o0 .. o0 + 3 of the two mask rows as one unaligned dword each (the mask buffer has slack behind its last row)
            const unsigned r0 = *(DG_GL const dg_uv1 *)(mm + rowOff + o0), r1 = *(DG_GL const dg_uv1 *)(mm + rowOff + B.XP + o0);
            auto vc = [&](int k) { return (int)(unsigned char)((((r0 >> (8 * k)) & 0xffu) * wt + ((r1 >> (8 * k)) & 0xffu) * wb + 8192) >> 14); };
            const int a0 = vc(0), a1 = vc(1), a2 = o0 + 2 < B.XP ? vc(2) : a1;
#pragma unroll
            for (int i = 0; i < W; i++) {
                const int o = hO[i], wr = hWr[i], wl = 16384 - wr, k = o - o0;
                int a, b;
                if (k == 0) { a = a0; b = a1; } else if (k == 1) { a = a1; b = a2; } else { a = vcol(mm, o); b = vcol(mm, o + 1); }
                mk[i] |= (unsigned)(unsigned char)((a * wl + b * wr + 8192) >> 14) << shift;
            }
        };
        if constexpr (MODE != 5) { upsize(m, 0); upsize(m + B.XP * B.YP, 8); }
        if constexpr (MODE >= 4) upsize(m + 2 * B.XP * B.YP, 16);
    }
    // one sample of a block from its two fetches
    auto value = [&](int i, unsigned b, unsigned fw) {
        return mvx_bff_value(MODE, t, __uint_as_float(sVal.d[i]), __uint_as_float(rVal.d[i]), __uint_as_float(b), __uint_as_float(fw), (int)(mk[i] & 0xffu),
                             (int)((mk[i] >> 8) & 0xffu), (int)(mk[i] >> 16));
    };
    DG_GL const unsigned char *pl = dg_gl(plan + (size_t)f * P.nBlk);
    DG_GL const unsigned char *refSup = dg_gl(J.refSup[p]), *srcSup = dg_gl(J.srcSup[p]);
    if (!P.overlap) { // blocks side by side (their sizes are powers of two): the value itself
        DgRaw<float, W> bv = sVal, fv = sVal; // (mode 5 reads neither)
        if constexpr (MODE != 5) {
            const int lbw = __ffs(g.blkW) - 1, lbh = __ffs(g.blkH) - 1;
            const int bx = x0 >> lbw, by = y >> lbh, px = x0 & (g.blkW - 1), py = y & (g.blkH - 1);
            const dg_iv4 R = *(DG_GL const dg_iv4 *)(pl + (size_t)(by * P.nBlkX + bx) * sizeof(BFPlan));
            const long long bo = (long long)py * g.supPitch + (long long)px * 4;
            bv = dg_load_raw<float, W>(refSup + (unsigned)R[c] + bo);
            fv = dg_load_raw<float, W>(srcSup + (unsigned)R[2 + c] + bo);
        }
#pragma unroll
        for (int i = 0; i < W; i++) { out.d[i] = __float_as_uint(value(i, bv.d[i], fv.d[i])); BFF_ONE_AT_A_TIME(); }
        bff_store<W>(dptr, out, W);
        return;
    }
    // overlapped blocks: the blocks bx0..bx1 x by0..by1 cover the cell, at most two each way, by outer and bx inner.  One block at a time: its
    // two fetches and its window row are all that is live beside the cell's own state, which keeps the kernel at cn_cell_kernel<float, W>'s occupancy
    int bx0, bx1, by0, by1;
    blk_cover(x0, g.blkW, g.stepX, P.nBlkX, bx0, bx1);
    blk_cover(y, g.blkH, g.stepY, P.nBlkY, by0, by1);
    DG_GL const unsigned char *win = dg_gl(P.win[p]);
    float acc[W];
    int wsum[W];
#pragma unroll
    for (int i = 0; i < W; i++) { acc[i] = 0.0f; wsum[i] = 0; }
#pragma unroll 1
    for (int by = by0; by <= by1; by++) {
        const int py = y - by * g.stepY, wrow = BLK_WIN_ROW(by, P.nBlkY);
#pragma unroll 1
        for (int bx = bx0; bx <= bx1; bx++) {
            const int px = x0 - bx * g.stepX; // 0 <= px <= blkW - W
            DgRaw<float, W> bv = sVal, fv = sVal; // (mode 5 reads neither)
            if constexpr (MODE != 5) {
                const dg_iv4 R = *(DG_GL const dg_iv4 *)(pl + (size_t)(by * P.nBlkX + bx) * sizeof(BFPlan));
                const long long bo = (long long)py * g.supPitch + (long long)px * 4;
                bv = dg_load_raw<float, W>(refSup + (unsigned)R[c] + bo);
                fv = dg_load_raw<float, W>(srcSup + (unsigned)R[2 + c] + bo);
            }
            const DgRaw<unsigned short, W> wv = dg_load_raw<unsigned short, W>(win + (size_t)((wrow + BLK_WIN_COL(bx, P.nBlkX)) * g.blkW * g.blkH + py * g.blkW + px) * 2);
#pragma unroll
            for (int i = 0; i < W; i++) {
                const int wi = dg_sample(wv, i);
                acc[i] = mvx_bff_add(acc[i], value(i, bv.d[i], fv.d[i]), wi);
                wsum[i] += wi;
                BFF_ONE_AT_A_TIME();
            }
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) out.d[i] = __float_as_uint(mvx_bff_out(acc[i], wsum[i]));
    bff_store<W>(dptr, out, W);
}

struct mvx_blockfps : DGCommon {
    BFParams B;
    DevBuf<BFParams> dB;
    DevBuf<BFJob> dBJobs;         // grows to twice the call's jobs, as do the masks
    DevBuf<int> dSmall, dTables;
    DevBuf<unsigned char> dMasks;
    FpsRate rate;
    int delta;
    bool flt = false;             // float super clip, float clip and output planes (bf_cell_float_kernel)
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
    DGParams &P = h->P;
    h->flt = flt;
    // P.bps stays the sample size (4: pitches, the plan's offsets, supInterior).  P.bits is read by bf_mask_kernel alone on this path, as the
    // depth of the SADs (sad >> (bits - 8)): that of the search, not the super clip's 32
    if (flt) P.bits = bw->bitsPerSample;
    if (!(si.modeYUV & 6)) P.nplanes = 1;
    P.nRefs = 2; P.thscd1 = thscd1; P.thscd2 = thscd2;
    fps_rate_init(h->rate, a->num, a->den, fps_num, fps_den, num_frames);
    h->delta = bw->nDeltaFrame;
    BFParams &B = h->B;
    memset(&B, 0, sizeof(B));
    B.mode = mode; B.blend = blend; B.ml = a->ml; B.thscd1 = thscd1; B.thscd2 = thscd2;
    fps_padded_grid(bw, &B.XP, &B.YP, B.nWidthP, B.nHeightP);
    const int bps = P.bps;
    B.supInterior[0] = si.hpad * bps + (int)super_pitch[0] * si.vpad;
    for (int p = 1; p < 3; p++) B.supInterior[p] = (si.hpad >> 1) * bps + (int)super_pitch[p < si.num_planes ? p : 0] * (si.vpad >> 1); // the reference's ">> 1" (:459-463)
    for (int p = 0; p < 3; p++) B.clipPitch[p] = clip_pitch[p < si.num_planes ? p : 0];
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

extern "C" __attribute__((visibility("default"))) int mvx_blockfps_frames(mvx_blockfps *b, int nframes, const mvx_blockfps_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    const DGParams &P = b->P;
    BFParams &B = b->B;
    for (int f = 0; f < nframes; f++) {
        const mvx_blockfps_job &J = jobs[f];
        if (!J.clip_left[0] || (J.time256 > 0 && !J.clip_right[0])) { mvx_set_error("mvx_blockfps_frames: clip_left / clip_right are required"); return MVX_E_ARG; }
        if (int rc = fps_check_planes("mvx_blockfps_frames", "clip_left", J.clip_left, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_blockfps_frames", "clip_right", J.clip_right, P.nplanes, P.bps, false)) return rc;
        if (int rc = fps_check_planes("mvx_blockfps_frames", "dst", J.dst, P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_blockfps_frames", "source super", J.src_super, P.nplanes, 16, false)) return rc;
        if (int rc = fps_check_planes("mvx_blockfps_frames", "reference super", J.ref_super, P.nplanes, 16, false)) return rc;
    }
    CallGuard::Scope scope(b->guard, st);
    int rc = blk_upload(b->dP, b->P, b->win);
    if (rc) return rc;
    if (!b->dB.p && (rc = fps_upload_tables(b->dTables, b->dB, B, B.nWidthP, B.nHeightP))) return rc;
    if ((rc = ensure_jobs(b, nframes, sizeof(BFPlan) * (size_t)P.nBlk))) return rc;
    const size_t n = (size_t)nframes, cells = (size_t)B.XP * B.YP;
    HIP_CHECK(b->dBJobs.reserve(n, n));
    HIP_CHECK(b->dSmall.reserve(n * 2 * cells, n * 2 * cells));
    HIP_CHECK(b->dMasks.reserve(n * 3 * cells + 16, n * 3 * cells)); // (+ slack: the row kernels read mask bytes four at a time)
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
    HIP_CHECK(hipMemcpyAsync(b->dBJobs.p, hj.data(), sizeof(BFJob) * nframes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bf_usable_kernel, dim3(nframes), dim3(256), 0, st, b->dP.p, b->dB.p, b->dBJobs.p, b->dUsable.p);
    if (B.mode >= 3) {
        HIP_CHECK(hipMemsetAsync(b->dSmall.p, 0, n * 2 * cells * sizeof(int), st));
        hipLaunchKernelGGL(bf_mask_kernel, dim3((P.nBlk + 255) / 256, 2, nframes), dim3(256), 0, st, b->dP.p, b->dB.p, b->dBJobs.p, b->dUsable.p, b->dSmall.p);
        hipLaunchKernelGGL(bf_mask_finish_kernel, dim3((unsigned)((cells + 255) / 256), nframes), dim3(256), 0, st, b->dP.p, b->dB.p, b->dUsable.p, b->dSmall.p, b->dMasks.p);
    }
    const BFPlan *plan = (const BFPlan *)b->dPlan.p;
    hipLaunchKernelGGL(bf_plan_kernel, dim3((P.nBlk + 255) / 256, nframes), dim3(256), 0, st, b->dP.p, b->dBJobs.p, b->dUsable.p, (BFPlan *)b->dPlan.p);
    if (b->flt) { // one launch for the luma planes of all jobs, one for both chroma planes
        // the widest cell at which the mode's kernel keeps occupancy 8: 16 bytes in modes 0, 5 and 8, 8 bytes in modes 1, 2, 3 and 6, one sample in
        // modes 4 and 7 (profiles/blockfps_float_isa.txt)
        const int m = B.mode < 6 ? B.mode : B.mode - 3, mw = m == 0 || m == 5 ? 4 : m == 4 ? 1 : 2;
        for (int cls = 0; cls < (P.nplanes > 1 ? 2 : 1); cls++) {
            const int p0 = cls, npl = cls ? 2 : 1, W = blk_cell_width(P.pl[p0], mw);
            const dim3 grid(((P.pl[p0].W + W - 1) / W + 31) / 32, (P.pl[p0].H + 7) / 8, nframes * npl);
#define BFF(N, M) hipLaunchKernelGGL((bf_cell_float_kernel<N, M>), grid, dim3(256), 0, st, b->dP.p, b->dB.p, b->dBJobs.p, b->dUsable.p, plan, b->dMasks.p, p0, npl)
#define BFW(M) switch (W) { case 1: BFF(1, M); break; case 2: BFF(2, M); break; default: BFF(4, M); break; }
#define BFN(M) switch (W) { case 1: BFF(1, M); break; default: BFF(2, M); break; }
            switch (m) { case 0: BFW(0); break; case 1: BFN(1); break; case 2: BFN(2); break; case 3: BFN(3); break; case 4: BFF(1, 4); break; default: BFW(5); break; }
#undef BFN
#undef BFW
#undef BFF
        }
        HIP_CHECK(hipGetLastError());
        return MVX_OK;
    }
    const int cwY = dg_rows_cw(P, 0), cwC = P.nplanes > 1 ? dg_rows_cw(P, 1) : 1;
    if (cwY && cwC && (P.nplanes == 1 || P.pl[1].W == P.pl[2].W)) {
        fps_classes(P.pl, P.nplanes, nframes, [&](int p) { return p ? cwC : cwY; }, [&](dim3 grid, int cw, int p0, int npl) {
            fps_dispatch<2>(P.bps, cw, [&](auto t, auto w) {
                hipLaunchKernelGGL((blockfps_rows_kernel<typename decltype(t)::type, decltype(w)::value>), grid, dim3(256), 0, st, b->dP.p, b->dB.p, b->dBJobs.p, b->dUsable.p, plan,
                                   b->dMasks.p, p0, npl);
            });
        });
    } else {
        dim3 grid((P.pl[0].W + 63) / 64, (P.pl[0].H + 3) / 4, nframes * 3);
        if (P.bps == 1) hipLaunchKernelGGL(blockfps_kernel<uint8_t>, grid, dim3(256), 0, st, b->dP.p, b->dB.p, b->dBJobs.p, b->dUsable.p, plan, b->dMasks.p);
        else hipLaunchKernelGGL(blockfps_kernel<uint16_t>, grid, dim3(256), 0, st, b->dP.p, b->dB.p, b->dBJobs.p, b->dUsable.p, plan, b->dMasks.p);
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
