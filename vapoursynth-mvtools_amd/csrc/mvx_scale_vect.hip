// mvx_scale_vect.hip -- ScaleVect on gfx950: the MVTools_vectors blobs of a vector clip rewritten for a clip `scale` (1, 2 or 4) times its
// size, so that vectors searched on a small (or 8-bit) clip can be used on the full-size one.  No reference counterpart: pinterf's MScaleVect
// is the model.  The contract is DESIGN.md 4.3.3 and include/mvtools_amd.h; tests/scale_vect_ref.py restates it in numpy.
//
// A blob is two header words, then per level (coarsest first) one size word and the level's records of 16 bytes (x, y, 64-bit SAD).  The
// scaled clip has the same block grid on every level (mvx_scale_vect_create checks it), so the layout does not change and the work is a
// stream: every record is read once and written once at the same offset.
//   scale_vect_kernel : ONE launch for all fields of all jobs.  A workgroup belongs to one (field, level): its 256 lanes take 256 consecutive
//                       records of that level, a wave reads and writes 1 KB of consecutive bytes.  The level comes out of a small table in the
//                       kernel arguments by the workgroup's number (uniform: scalar loads, no divergence); only level 0 needs the block's
//                       column and row, for the clamp into the block's legal rectangle on the target super clip.
// Records are 4-byte aligned and no more (the first level starts at byte 12 of the blob, every later one wherever the sizes before it
// put it), so a record is moved as four dwords.  A lane touches no byte outside its record (lane 0 of a field's first workgroup: the header
// and size words as well), which is what makes out == in legal.
#include "mvx_common.h"

#define SV_MOTION_USE_CHROMA_MOTION 8
#define SV_GL __attribute__((address_space(1)))

struct SVLevel {
    int firstGroup;   // the first workgroup of this level inside a field's share of the grid
    int nRec;         // records (blocks) of the level
    unsigned off;     // byte offset of the level's first record inside the blob; its size word is at off - 4
};

struct SVParams {
    int nLevels, groups;                  // levels of a blob; workgroups per field
    int m, sadMul, sadShift;              // x' = x * m; sad' = sad * sadMul << sadShift (>> -sadShift when negative)
    int nBlkX;                            // level 0
    int xMin0, xMax0, xStep, yMin0, yMax0, yStep; // legal rectangle of block (bx, by) of the scaled clip: [xMin0 - bx * xStep, xMax0 - bx * xStep], y alike
    SVLevel lv[MVX_MAX_LEVELS];           // lv[0] = level 0 (the finest, last in the blob), so most workgroups stop at the first comparison
};

struct SVField { const unsigned char *in; unsigned char *out; };

__device__ __forceinline__ int sv_clamp(long long v, int lo, int hi) { return (int)(v < lo ? lo : v > hi ? hi : v); }

__global__ __launch_bounds__(256) void scale_vect_kernel(const SVParams P, const SVField *fields) {
    const unsigned f = blockIdx.x / (unsigned)P.groups;
    const int g = (int)(blockIdx.x - f * (unsigned)P.groups);
    const SVField F = fields[f];
    SV_GL const unsigned *in = (SV_GL const unsigned *)(unsigned long long)F.in;
    SV_GL unsigned *out = (SV_GL unsigned *)(unsigned long long)F.out;
    int l = 0;
    while (l + 1 < P.nLevels && g >= P.lv[l + 1].firstGroup) l++;
    const SVLevel L = P.lv[l];
    const bool valid = in[1] != 0;
    if (g == 0 && threadIdx.x == 0 && F.in != F.out) { // the words that are not records: copied
        out[0] = in[0]; out[1] = in[1];
        for (int k = 0; k < P.nLevels; k++) { const unsigned w = P.lv[k].off / 4 - 1; out[w] = in[w]; }
    }
    const int i = (g - L.firstGroup) * 256 + (int)threadIdx.x;
    if (i >= L.nRec) return;
    const size_t w = L.off / 4 + (size_t)i * 4;
    unsigned r0 = in[w], r1 = in[w + 1], r2 = in[w + 2], r3 = in[w + 3];
    if (valid) {
        const long long x = (long long)(int)r0 * P.m, y = (long long)(int)r1 * P.m;
        unsigned long long sad = ((unsigned long long)r3 << 32 | r2) * (unsigned long long)P.sadMul; // two's complement: wraps
        sad = P.sadShift >= 0 ? sad << P.sadShift : (unsigned long long)((long long)sad >> -P.sadShift);
        if (l == 0) { // the consumers read level 0 only: it must stay inside the target super clip's padding
            const int by = i / P.nBlkX, bx = i - by * P.nBlkX;
            r0 = (unsigned)sv_clamp(x, P.xMin0 - bx * P.xStep, P.xMax0 - bx * P.xStep);
            r1 = (unsigned)sv_clamp(y, P.yMin0 - by * P.yStep, P.yMax0 - by * P.yStep);
        } else {
            r0 = (unsigned)x; r1 = (unsigned)y;
        }
        r2 = (unsigned)sad; r3 = (unsigned)(sad >> 32);
    }
    out[w] = r0; out[w + 1] = r1; out[w + 2] = r2; out[w + 3] = r3;
}

// ------------------------------------------------------------------------------------------------ host object

struct mvx_scale_vect {
    CallGuard guard;
    SVParams P;
    mvx_analysis_data out;
    size_t fieldSize = 0;          // bytes of a blob, before and after
    DevBuf<SVField> dFields;
};

extern "C" __attribute__((visibility("default"))) int mvx_vectors_size(const mvx_analysis_data *ad); // mvx_degrain.hip

extern "C" __attribute__((visibility("default"))) int mvx_scale_vect_create(const mvx_analysis_data *in, int scale, const mvx_super *target, mvx_scale_vect **out, char *err) {
    MVX_CREATE_BEGIN(out);
    MVX_REFUSE_FLOAT(target, "ScaleVect");
    const mvx_super_info &si = target->info;
    const int s = scale;
    if (s != 1 && s != 2 && s != 4) MVX_FAIL("ScaleVect: scale must be 1, 2 or 4.");
    if (si.width != s * in->nWidth || si.height != s * in->nHeight || si.super_width - 2 * si.hpad != s * in->nWidth)
        MVX_FAIL("ScaleVect: the target super clip must be scale times the size of the vectors' clip.");
    const bool chroma = (in->nMotionFlags & SV_MOTION_USE_CHROMA_MOTION) != 0;
    if (in->xRatioUV != si.xRatioUV || in->yRatioUV != si.yRatioUV || (chroma && (si.modeYUV & 6) != 6))
        MVX_FAIL("ScaleVect: the target super clip's chroma subsampling or colour data is not that of the vectors.");
    {
        static const int okb[12][2] = { { 4, 4 }, { 8, 4 }, { 8, 8 }, { 16, 2 }, { 16, 8 }, { 16, 16 }, { 32, 16 }, { 32, 32 }, { 64, 32 }, { 64, 64 }, { 128, 64 }, { 128, 128 } };
        bool found = false;
        for (auto &b : okb) found |= (s * in->nBlkSizeX == b[0] && s * in->nBlkSizeY == b[1]);
        if (!found) MVX_FAIL("ScaleVect: the scaled block size must be 4x4, 8x4, 8x8, 16x2, 16x8, 16x16, 32x16, 32x32, 64x32, 64x64, 128x64, or 128x128.");
    }
    if (in->nPel <= 0 || (s * si.pel) % in->nPel) MVX_FAIL("ScaleVect: scale times the target's pel must be a multiple of the vectors' pel.");
    const int m = s * si.pel / in->nPel;
    if (in->nLvCount < 1 || in->nLvCount > MVX_MAX_LEVELS || in->nBlkX < 1 || in->nBlkY < 1 || in->nOverlapX < 0 || in->nOverlapY < 0 ||
        in->nOverlapX >= in->nBlkSizeX || in->nOverlapY >= in->nBlkSizeY || in->bitsPerSample < 8 || in->bitsPerSample > 16)
        MVX_FAIL("ScaleVect: the vectors' analysis data is not that of a vector clip.");

    mvx_analysis_data o = *in;
    o.nBlkSizeX *= s; o.nBlkSizeY *= s; o.nOverlapX *= s; o.nOverlapY *= s; o.nWidth *= s; o.nHeight *= s;
    o.nPel = si.pel; o.bitsPerSample = si.bits; o.nHPadding = si.hpad; o.nVPadding = si.vpad;

    // the level grids, as mvx_vectors_size and every reader derive them (GroupOfPlanes.c:25-56), for both clips: they must agree
    SVParams P;
    memset(&P, 0, sizeof(P));
    const mvx_analysis_data *both[2] = { in, &o };
    int grid[2][MVX_MAX_LEVELS][2];
    for (int k = 0; k < 2; k++) {
        const mvx_analysis_data &a = *both[k];
        const int stepX = a.nBlkSizeX - a.nOverlapX, stepY = a.nBlkSizeY - a.nOverlapY;
        const int wB = stepX * a.nBlkX + a.nOverlapX, hB = stepY * a.nBlkY + a.nOverlapY;
        for (int i = 0; i < a.nLvCount; i++) {
            grid[k][i][0] = ((wB >> i) - a.nOverlapX) / stepX;
            grid[k][i][1] = ((hB >> i) - a.nOverlapY) / stepY;
        }
    }
    unsigned off = 8;
    for (int i = in->nLvCount - 1; i >= 0; i--) {
        if (grid[0][i][0] != grid[1][i][0] || grid[0][i][1] != grid[1][i][1] || grid[0][i][0] < 0 || grid[0][i][1] < 0)
            MVX_FAIL("ScaleVect: level %d of the scaled clip has another block grid than the vectors' (internal).", i);
        P.lv[i].nRec = grid[0][i][0] * grid[0][i][1];
        P.lv[i].off = off + 4;
        off += 4 + 16u * (unsigned)P.lv[i].nRec;
    }
    if ((int)off != mvx_vectors_size(in) || mvx_vectors_size(&o) != mvx_vectors_size(in))
        MVX_FAIL("ScaleVect: the scaled blob has another size than the vectors' (internal).");
    if (grid[0][0][0] != in->nBlkX || grid[0][0][1] != in->nBlkY) MVX_FAIL("ScaleVect: the vectors' analysis data is not that of a vector clip.");
    int groups = 0;
    for (int i = 0; i < in->nLvCount; i++) { P.lv[i].firstGroup = groups; groups += (P.lv[i].nRec + 255) / 256; }
    P.nLevels = in->nLvCount; P.groups = groups;
    P.m = m; P.sadMul = s * s; P.sadShift = si.bits - in->bitsPerSample;
    P.nBlkX = o.nBlkX;
    // tests/vector_fields.py legal_rect, oracle/mvo_analyse.c:580-583: -(pos + pad) * pel .. (size + pad - pos - blk) * pel - 1
    P.xStep = (o.nBlkSizeX - o.nOverlapX) * o.nPel; P.yStep = (o.nBlkSizeY - o.nOverlapY) * o.nPel;
    P.xMin0 = -o.nHPadding * o.nPel; P.xMax0 = (o.nWidth + o.nHPadding - o.nBlkSizeX) * o.nPel - 1;
    P.yMin0 = -o.nVPadding * o.nPel; P.yMax0 = (o.nHeight + o.nVPadding - o.nBlkSizeY) * o.nPel - 1;

    mvx_scale_vect *h = new mvx_scale_vect();
    h->P = P; h->out = o; h->fieldSize = off;
    *out = h;
    return MVX_OK;
}

extern "C" __attribute__((visibility("default"))) void mvx_scale_vect_destroy(mvx_scale_vect *h) { delete h; }
extern "C" __attribute__((visibility("default"))) void mvx_scale_vect_get_data(const mvx_scale_vect *h, mvx_analysis_data *out) { *out = h->out; }

extern "C" __attribute__((visibility("default"))) int mvx_scale_vect_frames(mvx_scale_vect *h, int njobs, const mvx_scale_vect_job *jobs, void *stream) {
    if (njobs <= 0) return MVX_OK;
    hipStream_t st = (hipStream_t)stream;
    const SVParams &P = h->P;
    std::vector<SVField> hf;
    for (int j = 0; j < njobs; j++) {
        const mvx_scale_vect_job &J = jobs[j];
        if (!J.in || !J.out || J.fields < 1) { mvx_set_error("mvx_scale_vect_frames: a job needs its input, its output and at least one field"); return MVX_E_ARG; }
        if (((uintptr_t)J.in | (uintptr_t)J.out) & 3) { mvx_set_error("mvx_scale_vect_frames: blobs must be 4-byte aligned"); return MVX_E_ARG; }
        if (J.fields > 1 && (J.field_stride < h->fieldSize || J.field_stride % 4)) {
            mvx_set_error("mvx_scale_vect_frames: field_stride must be a multiple of 4 and hold a field's %zu bytes", h->fieldSize);
            return MVX_E_ARG;
        }
        for (int r = 0; r < J.fields; r++)
            hf.push_back(SVField{ (const unsigned char *)J.in + (size_t)r * J.field_stride, (unsigned char *)J.out + (size_t)r * J.field_stride });
    }
    if (P.groups == 0) return MVX_OK;
    if (hf.size() > (size_t)0x7fffffff / (size_t)P.groups) { mvx_set_error("mvx_scale_vect_frames: at most %zu fields per call for this clip", (size_t)0x7fffffff / (size_t)P.groups); return MVX_E_ARG; }
    CallGuard::Scope scope(h->guard, st);
    HIP_CHECK(h->dFields.reserve(hf.size(), hf.size() / 2));
    HIP_CHECK(hipMemcpyAsync(h->dFields.p, hf.data(), sizeof(SVField) * hf.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(scale_vect_kernel, dim3((unsigned)(hf.size() * (size_t)P.groups)), dim3(256), 0, st, P, (const SVField *)h->dFields.p);
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}
