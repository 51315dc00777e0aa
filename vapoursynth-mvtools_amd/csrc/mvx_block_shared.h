// mvx_block_shared.h -- what the block filters share (mvx_degrain.hip: Degrain; mvx_degrain_n.hip: DegrainN; mvx_compensate.hip: Compensate,
// CompensateN; mvx_blockfps.hip: BlockFPS).
// All five read level-0 vectors, turn every block into an offset into a super plane, gather the up to 2 x 2 overlapped blocks that cover a
// cell, weigh them with the overlap windows and store.  Device side: which blocks cover a sample or a cell and which of the nine windows a
// block takes, and fgopIsUsable with the level-0 offset as its result (the N filters).  Host side: the geometry that opens every parameter
// block with its two checks, the overlap windows on the device, and the creation arguments that Degrain / DegrainN and Compensate /
// CompensateN resolve alike.  On top of mvx_fps_shared.h, which stays what ALL vector consumers share (the flow filters and mv.Mask have no
// blocks to gather); the wide sample loads and stores are there because those filters use them too.  Internal; not part of the ABI.
#pragma once
#include "mvx_fps_shared.h"
#include "mvx_degrain_n_weights.h"

// ------------------------------------------------------------------------------------------------ device

// what DGParams, DNParams, CNParams and BFParams open with (they derive from it, so the kernels read P.nBlkX as before)
struct BlkGeom {
    int nBlkX, nBlkY, nBlk, pel, logPel, bits, bps, nplanes, overlap;
    int nLvCount;            // levels in a blob; the level-0 record is found by walking the per-plane size headers like fgopUpdate (Fakery.c:112-123)
    long long thscd1; int thscd2;
    PlaneG pl[3];
    const int16_t *win[3];   // the nine overlap windows of each plane's blocks (mvx_over_windows)
};

// Which blocks cover a sample and which window a block takes.  The three expressions are macros and blk_cover takes the geometry by
// reference, so that a field is read where the expression uses it, as when it was written out in each kernel: with inline functions that
// take values the gather kernels compiled to other code, and degrain_cell_kernel did with every function form tried (VALU counts and
// registers moved in all its instantiations; profiles/block_shared_isa.txt).
// The first of the blocks of `size` samples, stepping by `step`, that cover sample x (or the cell that starts at x) along one axis
#define BLK_FIRST(x, size, step) ((x) - (size) + 1 <= 0 ? 0 : ((x) - (size) + (step)) / (step))
// ... and all of them, b0..b1, of the axis's n blocks
__device__ __forceinline__ void blk_cover(int x, const int &size, const int &step, const int &n, int &b0, int &b1) {
    b1 = x / step; if (b1 > n - 1) b1 = n - 1;
    b0 = BLK_FIRST(x, size, step);
}
// the window of block (bx, by) is number BLK_WIN_ROW + BLK_WIN_COL of the nine: first / middle / last along each axis
#define BLK_WIN_ROW(by, nBlkY) ((by) == 0 ? 0 : ((by) == (nBlkY) - 1 ? 6 : 3)) // ((by + nBlkY - 3) / (nBlkY - 2)) * 3, MVDegrains.cpp:256, MVCompensate.c:263
#define BLK_WIN_COL(bx, nBlkX) ((bx) == (nBlkX) - 1 ? 2 : ((bx) == 0 ? 0 : 1)) // MVDegrains.cpp:260-262,285, MVCompensate.c:267-269,297

// per (job, reference) of the N filters, n references per job: 0 when the reference's vectors are not usable (fgopIsUsable, or a reference
// frame outside the clip, which may have no blob at all), else the byte offset of level 0 inside the blob (a walk over the per-level size
// headers, done once here).  A template so that only the units that launch it hold it; the two tables by value in a struct, with which the
// walk runs in scalar registers (18 VGPRs; as two pointer arguments 22 and flat loads)
struct BlkTables { const unsigned char *const *refs, *const *blobs; }; // [job][reference][plane], [job][reference]
template <typename PARAMS>
__global__ __launch_bounds__(256) void blk_usable_kernel(const PARAMS *Pp, int n, BlkTables T, unsigned *lv0) {
    const BlkGeom &G = *Pp;
    const int k = blockIdx.y * n + blockIdx.x;
    const unsigned char *blob = T.blobs[k];
    const bool ok = fps_block_usable(blob, T.refs[(size_t)k * 3] != nullptr, G.nLvCount, G.nBlk, G.thscd1, G.thscd2);
    if (threadIdx.x == 0) lv0[k] = ok ? (unsigned)((const unsigned char *)mvx_level0(blob, G.nLvCount) - blob) : 0u;
}

// ------------------------------------------------------------------------------------------------ host

// samples per cell of a plane for the cell kernels of the N filters and of BlockFPS: the largest power of two up to `widest` that divides the block width and the block step
static int blk_cell_width(const PlaneG &g, int widest) {
    int w = widest;
    while (w > 1 && (g.blkW % w || g.stepX % w)) w >>= 1;
    return w;
}

struct BlkWin { DevBuf<int16_t> d[2]; int classes = 1; }; // a handle's overlap windows on the device: luma, chroma

// the geometry of a filter whose parameter block was zeroed, and the checks that are the library's own: the block grid, then the plane
// layouts (mvx_fps_shared.h).  src_what: what the filter calls the planes behind src_pitch; dst_bps: the sample size of the planes it writes
// where that is not the clip's (out16)
static int blk_fill(BlkGeom &G, BlkWin &win, const mvx_analysis_data *ad, const mvx_super_info &si, const ptrdiff_t src_pitch[3], const ptrdiff_t super_pitch[3],
                    const ptrdiff_t dst_pitch[3], char *err, const char *src_what = "src", int dst_bps = 0) {
    G.nBlkX = ad->nBlkX; G.nBlkY = ad->nBlkY; G.nBlk = ad->nBlkX * ad->nBlkY;
    G.pel = ad->nPel; G.logPel = ad->nPel == 4 ? 2 : ad->nPel == 2 ? 1 : 0;
    G.bits = si.bits; G.bps = (si.bits + 7) / 8; G.nplanes = si.num_planes;
    G.overlap = ad->nOverlapX > 0 || ad->nOverlapY > 0;
    if (G.overlap && (ad->nBlkX < 3 || ad->nBlkY < 3)) MVX_FAIL("overlap needs at least 3x3 blocks (window selection divides by nBlk-2).");
    G.nLvCount = ad->nLvCount;
    fps_fill_planes(G.pl, ad, si, src_pitch, super_pitch, dst_pitch);
    if (si.num_planes > 1 && super_pitch[1] != super_pitch[2]) MVX_FAIL("U and V super planes must share one pitch.");
    if (int rc = fps_check_super_pitches(si, super_pitch, err)) return rc;
    if (src_pitch) if (int rc = fps_check_pitches(src_what, G.pl, si.num_planes, src_pitch, G.bps, err)) return rc;
    if (int rc = fps_check_pitches("dst", G.pl, si.num_planes, dst_pitch, dst_bps ? dst_bps : G.bps, err)) return rc;
    win.classes = si.num_planes > 1 ? 2 : 1;
    return MVX_OK;
}

// a new handle H (members P, derived from BlkGeom, and win) with its geometry filled, or none
template <typename H> static int blk_new(H **h, const mvx_analysis_data *ad, const mvx_super_info &si, const ptrdiff_t src_pitch[3], const ptrdiff_t super_pitch[3],
                                         const ptrdiff_t dst_pitch[3], char *err, const char *src_what = "src", int dst_bps = 0) {
    *h = new H();
    memset(&(*h)->P, 0, sizeof((*h)->P));
    const int rc = blk_fill((*h)->P, (*h)->win, ad, si, src_pitch, super_pitch, dst_pitch, err, src_what, dst_bps);
    if (rc) { delete *h; *h = nullptr; }
    return rc;
}

// device state is created on first use so that argument validation works without a GPU: the windows per plane class, then the parameter
// block, which points at them (BlockFPS, whose block points at its upsizer tables too, uploads it itself)
static int blk_upload_windows(BlkGeom &P, BlkWin &win) {
    if (P.overlap) {
        for (int c = 0; c < win.classes; c++) {
            const PlaneG &g = P.pl[c];
            std::vector<int16_t> w(9 * g.blkW * g.blkH);
            mvx_over_windows(w.data(), g.blkW, g.blkH, g.ovX, g.ovY);
            HIP_CHECK(win.d[c].reserve(w.size()));
            HIP_CHECK(hipMemcpy(win.d[c].p, w.data(), w.size() * 2, hipMemcpyHostToDevice));
        }
        P.win[0] = win.d[0].p; P.win[1] = P.win[2] = win.d[1].p;
    }
    return MVX_OK;
}
template <typename PARAMS> static int blk_upload(DevBuf<PARAMS> &dP, PARAMS &P, BlkWin &win) {
    if (dP.p) return MVX_OK;
    if (int rc = blk_upload_windows(P, win)) return rc;
    return fps_upload_params(dP, P);
}

// ---- creation arguments after the filter's own first check (the radius).  `name` is the filter's name in the messages; the order of the
// checks is the reference's.

// Degrain1..6 (MVDegrains.cpp:511-809) and DegrainN.  Degrain is DegrainN without far thresholds: every distance then has the threshold of
// the first (dn_threshold), which is Degrain's thsad * nSCD1 / nSCD1_old.  out16: the limits are in units of the 16-bit output
enum { DG_PLAIN = 0, DG_OUT16 = 1, DG_FLOAT = 2 }; // kind: the clip's depth out / out16 / mvx_degrain_n_create_float (limits on the 8-bit scale)
struct DgResolved { mvx_degrain_n_info info; int YUVplanes, limit, limitc; int64_t thscd1; int32_t thscd2; };
static int dg_resolve(const char *name, const mvx_degrain_n_args *a, int kind, const mvx_analysis_data *ad, const mvx_super_info &si, DgResolved *r, char *err) {
    const int radius = a->radius;
    const int64_t t1 = a->thsad == MVX_UNSET ? 400 : a->thsad, t1c = a->thsadc == MVX_UNSET ? t1 : a->thsadc;
    const int64_t t2 = a->thsad2 == MVX_UNSET ? t1 : a->thsad2, t2c = a->thsadc2 == MVX_UNSET ? t1c : a->thsadc2;
    const int plane = a->plane == MVX_UNSET ? 4 : a->plane;
    if (plane < 0 || plane > 4) MVX_FAIL("%s: plane must be between 0 and 4 (inclusive).", name);
    static const int planes[5] = { 1, 2, 4, 6, 7 };
    r->YUVplanes = planes[plane];
    int64_t nSCD1_old;
    if (int rc = mvx_resolve_thscd(name, a->thscd1, a->thscd2, ad, &r->thscd1, &r->thscd2, err, &nSCD1_old)) return rc;
    memset(&r->info, 0, sizeof(r->info));
    r->info.radius = radius; r->info.nrefs = 2 * radius;
    // the scaled thresholds per distance; which argument reaches INT_MAX (MVDegrains.cpp:660-666): thsad, thsadc, then the far thresholds --
    // the entries in between lie between the near and the far one
    dn_threshold_table(t1, t2, radius, r->thscd1, nSCD1_old, r->info.thsad_d);
    dn_threshold_table(t1c, t2c, radius, r->thscd1, nSCD1_old, r->info.thsadc_d);
    auto over = [](const int64_t *t, int from, int to) { for (int d = from; d < to; d++) if (t[d] >= 2147483647LL) return true; return false; };
    const int64_t *ty = r->info.thsad_d, *tc = r->info.thsadc_d;
    const char *which = over(ty, 0, 1) ? "" : over(tc, 0, 1) ? "c" : over(ty, 1, radius) ? "2" : over(tc, 1, radius) ? "c2" : nullptr;
    if (which) MVX_FAIL("%s: with this block size and video format, thsad%s must not exceed %lld or some calculations would overflow.", name, which,
                        (long long)(2147483647LL * nSCD1_old / r->thscd1));
    if (!mvx_super_fits(ad, si, true)) MVX_FAIL("%s: wrong source or super clip frame size.", name);
    const bool out16 = kind == DG_OUT16;
    if (out16 && si.bits != 8) MVX_FAIL("%s: out16 needs an 8 bit clip.", name);
    if (kind == DG_FLOAT && si.bits != 32) MVX_FAIL("%s: the float entry needs a float super clip.", name);
    const int pixelMax = out16 ? 65535 : kind == DG_FLOAT ? 255 : (1 << si.bits) - 1;
    r->limit = a->limit == MVX_UNSET ? pixelMax : a->limit;
    r->limitc = a->limitc == MVX_UNSET ? r->limit : a->limitc;
    if (r->limit < 0 || r->limit > pixelMax) MVX_FAIL("%s: limit must be between 0 and %d (inclusive).", name, pixelMax);
    if (r->limitc < 0 || r->limitc > pixelMax) MVX_FAIL("%s: limitc must be between 0 and %d (inclusive).", name, pixelMax);
    return MVX_OK;
}
// ... into a geometry that blk_fill has filled
static void dg_apply(BlkGeom &G, const DgResolved &r, const mvx_super_info &si) {
    G.thscd1 = r.thscd1; G.thscd2 = r.thscd2;
    G.pl[0].process = !!(r.YUVplanes & 1);
    G.pl[1].process = !!(r.YUVplanes & 2 & si.modeYUV);
    G.pl[2].process = !!(r.YUVplanes & 4 & si.modeYUV);
    G.pl[0].limit = r.limit; G.pl[1].limit = G.pl[2].limit = r.limitc;
}

// Compensate (MVCompensate.c:419-575) and CompensateN
struct CompResolved { int scBehavior, time256, fields; long long thSAD; int64_t thscd1; int32_t thscd2; };
// not_float: a float entry was handed an integer super clip (said after the frame-size check)
static int comp_resolve(const char *name, const mvx_compensate_args *a, const mvx_analysis_data *ad, const mvx_super_info &si, CompResolved *r, char *err,
                        bool not_float = false) {
    r->scBehavior = a->scbehavior == MVX_UNSET ? 1 : !!a->scbehavior;
    r->thSAD = a->thsad == MVX_UNSET ? 10000 : a->thsad;
    const double time = a->time;
    if (time < 0.0 || time > 100.0) MVX_FAIL("%s: time must be between 0.0 and 100.0 (inclusive).", name);
    int64_t nSCD1_old;
    if (int rc = mvx_resolve_thscd(name, a->thscd1, a->thscd2, ad, &r->thscd1, &r->thscd2, err, &nSCD1_old)) return rc;
    r->thSAD = r->thSAD * r->thscd1 / nSCD1_old; // :521
    if (!mvx_super_fits(ad, si, true)) MVX_FAIL("%s: wrong source or super clip frame size.", name);
    if (not_float) MVX_FAIL("%s: the float entry needs a float super clip.", name);
    r->fields = a->fields != MVX_UNSET && a->fields;
    if (r->fields && ad->nPel < 2) MVX_FAIL("%s: fields option requires pel > 1.", name); // :514-517
    r->time256 = (int)(time * 256 / 100); // :560
    return MVX_OK;
}
// ... into a geometry that blk_fill has filled
static void comp_apply(BlkGeom &G, const CompResolved &r, const mvx_super_info &si) {
    G.thscd1 = r.thscd1; G.thscd2 = r.thscd2;
    if (!(si.modeYUV & 6)) G.nplanes = 1; // num_planes :147-149
}

