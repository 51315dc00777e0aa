// mvx_compensate.hip -- mv.Compensate and mv.CompensateN on gfx950, one engine.  CompensateN: the frames n - tr .. n + tr compensated onto
// frame n from one multi blob (mvtools_amd.h, "the multi blob"), in temporal order, the source in the middle.  Compensate is its single-field
// form: one field, one output per job, no centre, and the one thing CompensateN has no use for, a field shift per job.
//
// Every compensated output is one mv.Compensate result (MVCompensate.c:73-374; what the block filters share -- geometry, windows, creation
// arguments, the usable kernel, block cover, loads -- is in mvx_block_shared.h): fgopIsUsable per field, the
// block origin from the vector scaled by time or the block's own place when its SAD reaches thsad, overlaps_c / ToPixels
// (Overlap.cpp:143-158,335-356) in gather form, the uncovered strips and the scene-change fallback per scbehavior.  The shape of the work:
// a job is nFields fields (2 * tr; 1) and nOut output frames (2 * tr + 1; 1), so
//   usable  one launch over (field, job): 0, or the byte offset of level 0 inside the field's blob (blk_usable_kernel)
//   plan    one launch over (block, field x job): where the block comes from in the chosen super frame, luma and chroma
//   output  one launch per plane class over (cell, row, plane x output x job): a thread produces one row of a cell of W samples -- W
//           divides the block width and the block step, so the same <= 2 x 2 blocks cover all of them and each costs one vector load.
//           Blocks side by side, the uncovered strips, an unusable field and the centre are a single load and store of the same cell.
// Nothing is sized by tr at compile time: the tables (source planes, reference planes, field blobs, output planes) live in global memory,
// and what a workgroup needs of them -- it serves ONE plane of ONE output -- is uniform, so it is kept in scalar registers.
#include "mvx_block_shared.h"

// ------------------------------------------------------------------------------------------------ device structs

struct CNParams : BlkGeom {
    int tr, nFields, nOut;
    int time256, scBehavior;
    long long thSAD;
};

struct __attribute__((aligned(16))) CNRec { unsigned off[2]; int fromRef; int pad; }; // off[0] luma, off[1] chroma
static_assert(sizeof(CNRec) == 16, "plan record layout");

// the tables of a call, all in one device block: [job][plane] | [job][field][plane] | [job][field] | [job][output][plane] | [job][output] | [job][field]
struct CNTables {
    const unsigned char *const *src;
    const unsigned char *const *refs;
    const unsigned char *const *blobs;
    unsigned char *const *dst;
    const int2 *out;         // per (job, output), the host's output -> field map: x the job, y the (job, field) row job * nFields + field, -1 for the centre
    const int *shift;        // added to a block's row in the super frame (MVCompensate.c:188-225; Compensate with fields = 1, else 0)
};

// output k of a job -> the field that compensates it, -1 for the centre: mvfw (odd fields) of distance tr - k before it, mvbw (even fields) of
// distance k - tr behind it
__host__ __device__ __forceinline__ int cn_field(int tr, int k) { return k == tr ? -1 : k < tr ? 2 * (tr - k - 1) + 1 : 2 * (k - tr - 1); }

// ------------------------------------------------------------------------------------------------ kernels

// one thread per (job x field, block): where the block comes from (MVCompensate.c:238-247,286-295).  The field shift moves the row in both
// cases: a block whose SAD reaches thsad is read from the source super frame at the shifted row too
__global__ __launch_bounds__(256) void cn_plan_kernel(const CNParams *Pp, CNTables T, const unsigned *lv0, CNRec *plan) {
    const CNParams &P = *Pp;
    const int k = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned l0 = lv0[k];
    if (i >= P.nBlk || !l0) return; // (the output kernel does not read the plan of a field that is not usable)
    const int by = i / P.nBlkX, bx = i - by * P.nBlkX;
    typedef unsigned pl_v4 __attribute__((ext_vector_type(4), aligned(4)));
    const pl_v4 v = *(DG_GL const pl_v4 *)(dg_gl(T.blobs[k]) + l0 + (size_t)i * sizeof(GVecD));
    const int vx = (int)v[0], vy = (int)v[1];
    const long long sad = (long long)(((unsigned long long)v[3] << 32) | v[2]);
    int blx = bx * P.pl[0].stepX * P.pel, bly = by * P.pl[0].stepY * P.pel + T.shift[k];
    CNRec rec;
    rec.fromRef = sad < P.thSAD;
    if (rec.fromRef) { blx += vx * P.time256 / 256; bly += vy * P.time256 / 256; }
    rec.off[0] = sup_offset(P.pl[0], P.pel, P.logPel, P.bps, blx, bly);
    rec.off[1] = P.nplanes > 1 ? sup_offset(P.pl[1], P.pel, P.logPel, P.bps, blx >> P.pl[1].subX, bly >> P.pl[1].subY) : 0;
    rec.pad = 0;
    plan[(size_t)k * P.nBlk + i] = rec;
}

// W * 4 bytes, 16 at most
template <int W> __device__ __forceinline__ void cn_store_raw(DG_GL unsigned char *p, const DgRaw<float, W> &r) {
    if constexpr (W == 4) { dg_uv4 t = { r.d[0], r.d[1], r.d[2], r.d[3] }; *(DG_GL dg_uv4 *)p = t; }
    else if constexpr (W == 2) { dg_uv2 t = { r.d[0], r.d[1] }; *(DG_GL dg_uv2 *)p = t; }
    else *(DG_GL dg_uv1 *)p = r.d[0];
}

// One thread per row of a cell; 256 threads = 32 cells x 8 rows of one plane of one output of one job.  z = (job, output, plane of the class).
// T: uint8_t, uint16_t, or float (mvx_compensate_n_create_float, mvx_compensate_create_float): the same cells and threads on float32 samples.
// Usable pass, plan and tables touch no sample, and every case but overlapped blocks moves the cell's bytes and never looks at them; what
// differs by T is the arithmetic of overlapped blocks.  Float is DegrainN-float's rule (include/mvtools_amd.h):
// acc = acc + v * (float)win over the covering blocks, by outer and bx inner, then acc / (float)wsum -- every operation rounded on its
// own, no shift, no rounding term, no clamp.
template <typename T, int W>
__global__ __launch_bounds__(256)
void cn_cell_kernel(const CNParams P, CNTables Tb, const unsigned *lv0, const CNRec *plan, int planeFirst, int planesPerFrame) {
    constexpr bool FLT = sizeof(T) == 4;
    static_assert(W * sizeof(T) <= 16, "cells of 16 bytes at most");
    const int z = blockIdx.z, p = planeFirst + (z & (planesPerFrame - 1)), zo = z >> (planesPerFrame - 1); // (a class has one plane or two)
    const PlaneG &g = P.pl[p];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    const int x0 = c * W;
    // uniform over the workgroup: which job and which of its fields, by the host's table -- no division by the output count here
    const int2 o = Tb.out[zo];
    const int f = o.x, row = o.y;
    const size_t anyRow = row >= 0 ? row : 0; // (the centre reads field 0's entries and uses neither)
    const unsigned char *srcSup = Tb.src[(size_t)f * 3 + p];
    const unsigned char *refAny = Tb.refs[anyRow * 3 + p];
    const unsigned lv0Any = lv0[anyRow];
    unsigned char *dstPlane = Tb.dst[(size_t)zo * 3 + p];
    // Read ahead of every branch, in two rounds: the parameters (kernel arguments, P by value), then the table entries.  Left to where
    // they are used these scalar loads come one by one, each behind its own wait, a dozen round trips before the first vector load of a
    // thread that moves 4 to 16 bytes; with them the side-by-side cells miss the speed of the row kernel they replaced and CompensateN is
    // 6 to 11 % slower (profiles/compensate_single_bench.txt).  CN_PIN makes the values exist here: an empty asm that takes them in
    // scalar registers.  Every pinned value depends on blockIdx and kernel arguments alone.  For a value that differed between lanes the
    // compiler would pass the asm the first lane's copy, silently; the asm ignores it and the code below reads the field again, so even
    // then results could not change -- only the point of the pin would be lost.
#define CN_PIN(...) asm volatile("" :: __VA_ARGS__)
    CN_PIN("s"(P.scBehavior), "s"(P.overlap), "s"(P.pel), "s"(P.nBlkX), "s"(P.nBlk));
    CN_PIN("s"(g.W), "s"(g.H), "s"(g.WB), "s"(g.HB), "s"(g.blkW), "s"(g.blkH), "s"(g.vpadPel), "s"(g.hpadPel), "s"(g.supPitch), "s"(g.dstPitch));
    CN_PIN("s"(srcSup), "s"(refAny), "s"(lv0Any), "s"(dstPlane));
#undef CN_PIN
    if (x0 >= g.W || y >= g.H) return;
    const unsigned char *refSup = row >= 0 ? refAny : nullptr;
    const bool usable = row >= 0 && lv0Any != 0u;
    unsigned char *drow = dstPlane + (long long)y * g.dstPitch + (long long)x0 * (long long)sizeof(T);
    // interior (pel plane 0) sample of a super frame
    const long long inner = (long long)(g.vpadPel / P.pel + y) * g.supPitch + (long long)(g.hpadPel / P.pel + x0) * (long long)sizeof(T);
    const bool covered = x0 < g.WB && y < g.HB; // (the covered width is a multiple of W: a cell that starts inside it lies inside it, and inside the frame)
    const unsigned char *sp = nullptr; // where a cell that is a plain copy comes from
    if (row < 0) sp = srcSup + inner;                                                           // the centre: the source
    else if (!usable) sp = ((!P.scBehavior && refSup) ? refSup : srcSup) + inner;               // MVCompensate.c:348-364
    else if (!covered) sp = (P.scBehavior ? srcSup : refSup) + inner;                           // :319-342
    else if (!P.overlap) {                                                                      // :227-258: plain block copies (block sizes are powers of two)
        const int lbw = __ffs(g.blkW) - 1, lbh = __ffs(g.blkH) - 1;
        const int bx = x0 >> lbw, by = y >> lbh, px = x0 & (g.blkW - 1), py = y & (g.blkH - 1);
        const dg_iv4 R = *(DG_GL const dg_iv4 *)dg_gl(plan + (size_t)row * P.nBlk + by * P.nBlkX + bx);
        sp = (R[2] ? refSup : srcSup) + (unsigned)R[p ? 1 : 0] + (long long)py * g.supPitch + (long long)px * (long long)sizeof(T);
    }
    if (sp) {
        if (x0 + W <= g.W) {
            if constexpr (FLT) cn_store_raw<W>(dg_glw(drow), dg_load_raw<float, W>(dg_gl(sp))); // the bytes as they are: no float operation sees them
            else { int v[W]; dg_load<T, W>(dg_gl(sp), v); dg_store<T, W>(dg_glw(drow), v); }
        } else {
            typedef typename std::conditional<FLT, unsigned, T>::type B;
#pragma unroll
            for (int i = 0; i < W; i++) if (x0 + i < g.W) ((B *)drow)[i] = ((const B *)sp)[i];
        }
        return;
    }
    // overlapped blocks (:260-317): the blocks bx0..bx1 x by0..by1 cover the cell, at most two each way (the overlap is at most half a block).
    // All four slots are loaded -- one that does not exist repeats the first and is left out -- so that the four plan records, and then the
    // four rows and window rows, are in flight together.
    int bx0, bx1, by0, by1;
    blk_cover(x0, g.blkW, g.stepX, P.nBlkX, bx0, bx1);
    blk_cover(y, g.blkH, g.stepY, P.nBlkY, by0, by1);
    DG_GL const unsigned char *pl = dg_gl(plan + (size_t)row * P.nBlk);
    DG_GL const unsigned char *win = dg_gl(P.win[p]);
    bool have[4];
    dg_iv4 R[4];
    int px[4], py[4], wsel[4];
#pragma unroll
    for (int s = 0; s < 4; s++) { // slot order: (by0, bx0), (by0, bx1), (by1, bx0), (by1, bx1)
        const int by = by0 + (s >> 1), bx = bx0 + (s & 1);
        have[s] = by <= by1 && bx <= bx1;
        const int byc = have[s] ? by : by0, bxc = have[s] ? bx : bx0;
        R[s] = *(DG_GL const dg_iv4 *)(pl + (size_t)(byc * P.nBlkX + bxc) * sizeof(CNRec));
        px[s] = x0 - bxc * g.stepX; py[s] = y - byc * g.stepY; // 0 <= px <= blkW - W
        wsel[s] = (BLK_WIN_ROW(byc, P.nBlkY) + BLK_WIN_COL(bxc, P.nBlkX)) * g.blkW * g.blkH + py[s] * g.blkW + px[s];
    }
#define CN_SLOT_ROW(s) ((R[s][2] ? refSup : srcSup) + (unsigned)R[s][p ? 1 : 0] + (long long)py[s] * g.supPitch + (long long)px[s] * (long long)sizeof(T))
    if constexpr (FLT) {
        DgRaw<float, W> val[4], out;
        DgRaw<unsigned short, W> wv[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            val[s] = dg_load_raw<float, W>(dg_gl(CN_SLOT_ROW(s)));
            wv[s] = dg_load_raw<unsigned short, W>(win + (size_t)wsel[s] * 2);
        }
#pragma unroll
        for (int i = 0; i < W; i++) {
            float acc = 0.0f;
            int wsum = 0;
#pragma unroll
            for (int s = 0; s < 4; s++) { // a missing slot by a select, never with weight 0: 0 * x is not 0 for the non-finite bytes that may lie behind a plane
                const int wi = dg_sample(wv[s], i);
                const float t = acc + __uint_as_float(val[s].d[i]) * (float)wi;
                acc = have[s] ? t : acc;
                wsum += have[s] ? wi : 0;
            }
            out.d[i] = __float_as_uint(acc / (float)wsum);
        }
        cn_store_raw<W>(dg_glw(drow), out);
    } else {
        int val[4][W], wv[4][W], out[W];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            dg_load<T, W>(dg_gl(CN_SLOT_ROW(s)), val[s]);
            dg_load<unsigned short, W>(win + (size_t)wsel[s] * 2, wv[s]);
        }
        const int pm = (1 << P.bits) - 1;
#pragma unroll
        for (int i = 0; i < W; i++) {
            unsigned acc = 0;
#pragma unroll
            for (int s = 0; s < 4; s++) acc += have[s] ? (unsigned)((val[s][i] * wv[s][i]) >> 6) : 0u; // overlaps_c, Overlap.cpp:143-158
            if (sizeof(T) == 1) acc &= 0xffffu; // 16-bit accumulator of the 8-bit path (Overlap.cpp:254-256)
            const int a = (int)((acc + 16) >> 5); // ToPixels, Overlap.cpp:335-356
            out[i] = a > pm ? pm : a;
        }
        dg_store<T, W>(dg_glw(drow), out);
    }
#undef CN_SLOT_ROW
}

// ------------------------------------------------------------------------------------------------ host object

// the object behind both handles of the header
struct CNObject {
    CallGuard guard;
    CNParams P;
    int minStride = 0;               // bytes of a field's blob
    DevBuf<CNParams> dP;
    DevBuf<unsigned char> dTables;   // per call: see CNTables
    DevBuf<unsigned> dLv0;
    DevBuf<CNRec> dPlan;
    BlkWin win;
    bool single = false;             // Compensate: output k is field k (one field, no centre); else cn_field(tr, k)
    bool flt = false;                // float super clip, float output planes (cn_cell_kernel<float, W>)
};
struct mvx_compensate_n : CNObject {};
struct mvx_compensate : CNObject {};

// MVCompensate.c:419-575 mvcompensateCreate.  single: Compensate -- one field, one output per job, no centre; else CompensateN, which says so
// in its messages.  flt: the float entries (the super clip must be a float one; said after the frame-size check)
template <typename H>
static int cn_create(const mvx_compensate_args *a, int tr, bool flt, bool single, const mvx_analysis_data *ad, const mvx_super *sup, const ptrdiff_t super_pitch[3],
                     const ptrdiff_t dst_pitch[3], H **out, char *err) {
    MVX_CREATE_BEGIN(out);
    const char *name = single ? "Compensate" : "CompensateN";
    if (!flt) MVX_REFUSE_FLOAT(sup, name);
    const mvx_super_info &si = sup->info;
    if (!single && (tr < 1 || tr > MVX_DEGRAIN_N_MAX_RADIUS)) MVX_FAIL("%s: tr must be between 1 and %d.", name, MVX_DEGRAIN_N_MAX_RADIUS);
    CompResolved r;
    if (int rc = comp_resolve(name, a, ad, si, &r, err, flt && !sup->is_float)) return rc;
    if (r.fields && single && flt) MVX_FAIL("%s: fields is not supported on float clips.", name);
    if (r.fields && !single) MVX_FAIL("%s: fields is not supported.", name);
    H *h;
    if (int rc = blk_new(&h, ad, si, nullptr, super_pitch, dst_pitch, err)) return rc;
    CNParams &P = h->P;
    P.tr = single ? 0 : tr; P.nFields = single ? 1 : 2 * tr; P.nOut = single ? 1 : 2 * tr + 1;
    h->single = single;
    P.thSAD = r.thSAD; P.time256 = r.time256; P.scBehavior = r.scBehavior;
    comp_apply(P, r, si);
    h->minStride = mvx_vectors_size(ad);
    h->flt = flt;
    *out = h;
    return MVX_OK;
}

extern "C" __attribute__((visibility("default"))) int mvx_compensate_create(const mvx_compensate_args *a, const mvx_analysis_data *ad, const mvx_super *sup,
                                                                            const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3], mvx_compensate **out, char *err) {
    return cn_create(a, 0, false, true, ad, sup, super_pitch, dst_pitch, out, err);
}
extern "C" __attribute__((visibility("default"))) int mvx_compensate_create_float(const mvx_compensate_args *a, const mvx_analysis_data *ad, const mvx_super *sup,
                                                                                  const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3], mvx_compensate **out, char *err) {
    return cn_create(a, 0, true, true, ad, sup, super_pitch, dst_pitch, out, err);
}
extern "C" __attribute__((visibility("default"))) int mvx_compensate_n_create(const mvx_compensate_args *a, int tr, const mvx_analysis_data *ad, const mvx_super *sup,
                                                                              const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3], mvx_compensate_n **out, char *err) {
    return cn_create(a, tr, false, false, ad, sup, super_pitch, dst_pitch, out, err);
}
extern "C" __attribute__((visibility("default"))) int mvx_compensate_n_create_float(const mvx_compensate_args *a, int tr, const mvx_analysis_data *ad, const mvx_super *sup,
                                                                                    const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3], mvx_compensate_n **out, char *err) {
    return cn_create(a, tr, true, false, ad, sup, super_pitch, dst_pitch, out, err);
}

extern "C" __attribute__((visibility("default"))) void mvx_compensate_destroy(mvx_compensate *c) { delete c; }
extern "C" __attribute__((visibility("default"))) void mvx_compensate_n_destroy(mvx_compensate_n *c) { delete c; }

extern "C" __attribute__((visibility("default"))) int mvx_compensate_n_map(const mvx_compensate_n *c, int k, int *offset, int *field) {
    if (k < 0 || k > 2 * c->P.tr) { mvx_set_error("mvx_compensate_n_map: output %d of %d", k, 2 * c->P.tr + 1); return MVX_E_ARG; }
    if (offset) *offset = k - c->P.tr;
    if (field) *field = cn_field(c->P.tr, k);
    return MVX_OK;
}

template <typename T> static void cn_launch_cells(int W, dim3 grid, hipStream_t st, const CNParams &P, const CNTables &tables, const unsigned *lv0, const CNRec *plan, int p0, int npl) {
#define CNC(N) hipLaunchKernelGGL((cn_cell_kernel<T, N>), grid, dim3(256), 0, st, P, tables, lv0, plan, p0, npl)
    switch (W) {
    case 1: CNC(1); break;
    case 2: CNC(2); break;
    case 4: CNC(4); break;
    case 8: if constexpr (sizeof(T) <= 2) CNC(8); break;
    default: if constexpr (sizeof(T) == 1) CNC(16); break; // (a cell is 16 bytes at most)
    }
#undef CNC
}

// a grid's y and z hold 65535: the output kernel's z is (job, output, chroma plane), the plan kernel's y (job, field)
static int cn_max_jobs(const CNParams &P) { return 65535 / (P.nOut * 2); }

// The launches of a call whose jobs have been checked.  fill(f, src, refs, blobs, dst, shift) writes job f's rows of the five tables, which
// are zeroed: [plane], [field][plane], [field], [output][plane], [field]
template <typename FILL> static int cn_run(CNObject *c, int njobs, hipStream_t st, FILL fill) {
    const CNParams &P = c->P;
    const size_t n = (size_t)njobs, nf = (size_t)P.nFields, no = (size_t)P.nOut;
    CallGuard::Scope scope(c->guard, st);
    int rc = blk_upload(c->dP, c->P, c->win);
    if (rc) return rc;
    // one host block, one copy (each part but the last a multiple of 8 bytes)
    const size_t offRefs = sizeof(void *) * 3 * n, offBlobs = offRefs + sizeof(void *) * 3 * nf * n, offDst = offBlobs + sizeof(void *) * nf * n,
                 offOut = offDst + sizeof(void *) * 3 * no * n, offShift = offOut + sizeof(int2) * no * n, total = offShift + sizeof(int) * nf * n;
    std::vector<unsigned char> host(total, 0);
    const unsigned char **hs = (const unsigned char **)host.data(), **hr = (const unsigned char **)(host.data() + offRefs),
                        **hb = (const unsigned char **)(host.data() + offBlobs);
    unsigned char **hd = (unsigned char **)(host.data() + offDst);
    int *hsh = (int *)(host.data() + offShift);
    int2 *ho = (int2 *)(host.data() + offOut);
    for (size_t f = 0; f < n; f++) {
        fill(f, hs + f * 3, hr + f * nf * 3, hb + f * nf, hd + f * no * 3, hsh + f * nf);
        for (size_t k = 0; k < no; k++) {
            const int field = c->single ? (int)k : cn_field(P.tr, (int)k);
            ho[f * no + k] = int2{ (int)f, field < 0 ? -1 : (int)(f * nf) + field };
        }
    }
    HIP_CHECK(c->dTables.reserve(total, total));
    HIP_CHECK(c->dLv0.reserve(nf * n, nf * n));
    HIP_CHECK(c->dPlan.reserve((size_t)P.nBlk * nf * n, (size_t)P.nBlk * nf * n / 2));
    HIP_CHECK(hipMemcpyAsync(c->dTables.p, host.data(), total, hipMemcpyHostToDevice, st));
    CNTables T;
    T.src = (const unsigned char *const *)c->dTables.p;
    T.refs = (const unsigned char *const *)(c->dTables.p + offRefs);
    T.blobs = (const unsigned char *const *)(c->dTables.p + offBlobs);
    T.dst = (unsigned char *const *)(c->dTables.p + offDst);
    T.out = (const int2 *)(c->dTables.p + offOut);
    T.shift = (const int *)(c->dTables.p + offShift);
    hipLaunchKernelGGL(blk_usable_kernel<CNParams>, dim3(P.nFields, njobs), dim3(256), 0, st, c->dP.p, P.nFields, BlkTables{T.refs, T.blobs}, c->dLv0.p);
    hipLaunchKernelGGL(cn_plan_kernel, dim3((P.nBlk + 255) / 256, njobs * P.nFields), dim3(256), 0, st, c->dP.p, T, c->dLv0.p, c->dPlan.p);
    for (int cls = 0; cls < (P.nplanes > 1 ? 2 : 1); cls++) { // one launch for the luma planes of all outputs of all jobs, one for both chroma planes
        const int p0 = cls, npl = cls ? 2 : 1, W = blk_cell_width(P.pl[p0], 16 / P.bps);
        const dim3 grid(((P.pl[p0].W + W - 1) / W + 31) / 32, (P.pl[p0].H + 7) / 8, njobs * P.nOut * npl);
        if (c->flt) cn_launch_cells<float>(W, grid, st, P, T, c->dLv0.p, c->dPlan.p, p0, npl);
        else if (P.bps == 1) cn_launch_cells<uint8_t>(W, grid, st, P, T, c->dLv0.p, c->dPlan.p, p0, npl);
        else cn_launch_cells<uint16_t>(W, grid, st, P, T, c->dLv0.p, c->dPlan.p, p0, npl);
    }
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}

// a reference outside the clip (plane 0 null) leaves its row of the table zeroed
static void cn_fill_ref(const unsigned char **row, const void *const planes[3], int nplanes) {
    if (planes[0]) for (int p = 0; p < nplanes; p++) row[p] = (const unsigned char *)planes[p];
}

extern "C" __attribute__((visibility("default"))) int mvx_compensate_n_frames(mvx_compensate_n *c, int njobs, const mvx_compensate_n_job *jobs, void *stream) {
    if (njobs <= 0) return MVX_OK;
    const CNParams &P = c->P;
    const size_t nf = (size_t)P.nFields, no = (size_t)P.nOut;
    if (njobs > cn_max_jobs(P)) { mvx_set_error("mvx_compensate_n_frames: at most %d jobs per call at tr %d", cn_max_jobs(P), P.tr); return MVX_E_ARG; }
    for (int f = 0; f < njobs; f++) {
        const mvx_compensate_n_job &J = jobs[f];
        if (!J.refs || !J.dst || !J.blob || !J.src_super[0]) { mvx_set_error("mvx_compensate_n_frames: a job needs its source, its reference table, its blob and its output table"); return MVX_E_ARG; }
        if (J.field_stride < (size_t)c->minStride || J.field_stride % 16) { mvx_set_error("mvx_compensate_n_frames: field_stride must be a multiple of 16 and hold a field's %d bytes", c->minStride); return MVX_E_ARG; }
        for (size_t k = 0; k < no; k++)
            for (int p = 0; p < P.nplanes; p++)
                if (!J.dst[k][p]) { mvx_set_error("mvx_compensate_n_frames: output %d lacks plane %d", (int)k, p); return MVX_E_ARG; }
        for (size_t k = 0; k < no; k++)
            if (int rc = fps_check_planes("mvx_compensate_n_frames", "dst", J.dst[k], P.nplanes, P.bps, true)) return rc;
        if (int rc = fps_check_planes("mvx_compensate_n_frames", "source super", J.src_super, P.nplanes, 16, true)) return rc;
        for (size_t r = 0; r < nf; r++)
            if (int rc = fps_check_planes("mvx_compensate_n_frames", "reference super", J.refs[r], P.nplanes, 16, false)) return rc;
    }
    return cn_run(c, njobs, (hipStream_t)stream, [&](size_t f, const unsigned char **src, const unsigned char **refs, const unsigned char **blobs, unsigned char **dst, int *) {
        const mvx_compensate_n_job &J = jobs[f];
        for (int p = 0; p < P.nplanes; p++) src[p] = (const unsigned char *)J.src_super[p];
        for (size_t r = 0; r < nf; r++) {
            cn_fill_ref(refs + r * 3, J.refs[r], P.nplanes);
            blobs[r] = (const unsigned char *)J.blob + r * J.field_stride;
        }
        for (size_t k = 0; k < no; k++)
            for (int p = 0; p < P.nplanes; p++) dst[k * 3 + p] = (unsigned char *)J.dst[k][p];
    });
}

// A job is a job of the engine with tables of one row each.  A job whose reference lies outside the clip needs no blob (the usable pass looks
// at the reference first), and the shell sends such jobs at the clip's ends; the float object has always asked for one.
extern "C" __attribute__((visibility("default"))) int mvx_compensate_frames(mvx_compensate *c, int nframes, const mvx_compensate_job *jobs, void *stream) {
    if (nframes <= 0) return MVX_OK;
    const CNParams &P = c->P;
    if (nframes > cn_max_jobs(P)) { mvx_set_error("mvx_compensate_frames: at most %d jobs per call%s", cn_max_jobs(P), c->flt ? " on float clips" : ""); return MVX_E_ARG; }
    for (int f = 0; f < nframes; f++) {
        if (c->flt && jobs[f].field_shift) { mvx_set_error("mvx_compensate_frames: field_shift is not supported on float clips"); return MVX_E_ARG; }
        if (c->flt && !jobs[f].blob) { mvx_set_error("mvx_compensate_frames: a job needs its blob"); return MVX_E_ARG; }
        if (int rc = fps_check_planes("mvx_compensate_frames", "source super", jobs[f].src_super, P.nplanes, 16, true)) return rc;
        if (int rc = fps_check_planes("mvx_compensate_frames", "reference super", jobs[f].ref_super, P.nplanes, 16, false)) return rc;
        if (int rc = fps_check_planes("mvx_compensate_frames", "dst", jobs[f].dst, P.nplanes, P.bps, true)) return rc;
    }
    return cn_run(c, nframes, (hipStream_t)stream, [&](size_t f, const unsigned char **src, const unsigned char **refs, const unsigned char **blobs, unsigned char **dst, int *shift) {
        const mvx_compensate_job &J = jobs[f];
        for (int p = 0; p < P.nplanes; p++) { src[p] = (const unsigned char *)J.src_super[p]; dst[p] = (unsigned char *)J.dst[p]; }
        cn_fill_ref(refs, J.ref_super, P.nplanes);
        blobs[0] = (const unsigned char *)J.blob;
        shift[0] = J.field_shift;
    });
}
