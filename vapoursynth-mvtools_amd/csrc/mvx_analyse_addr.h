// mvx_analyse_addr.h -- the reference addressing of the search kernels that form "uniform 64-bit level base + unsigned 32-bit byte offset"
// (the lean kernel, mvx_analyse_fast.h; the speculative kernel, mvx_analyse_spec.h; the specialised general kernels, mvx_analyse_kernel.h),
// for device and host.  One text: the kernels take their offsets from here, tests/search_addressing_host_main.cpp walks the same functions
// on the host over every level, block and loadable vector of a geometry and compares every piece address with the signed 64-bit truth
// (tests/test_search_addressing.py).  Internal; not part of the ABI.
//
// THE RULE.  The reference evaluates a CLIPPED predictor -- zero, global, hierarchical, left / up / ahead -- without asking
// whether it is legal (PlaneOfBlocks.cpp:859 ff.), and the clip is min(max(v, nDxMin), nDxMax - 1).  On a level whose size was floored below
// its block grid (pad smaller than the chroma ratio) the legal rectangle of a block can be EMPTY, the clip then returns nDxMax - 1 < nDxMin,
// and the block is read up to a few samples LEFT of and a few rows ABOVE the level's first sample -- inside the super frame (a coarser level
// lies behind the finer ones), but at a negative offset from the level base.  An unsigned 32-bit offset cannot say that: it wraps to
// 2^32 - something and the load lands 4 GiB behind the plane.  So every 32-bit offset is formed for a block origin moved by
// MVX_REF_BIAS_ROWS rows and MVX_REF_BIAS_COLS samples, and the kernels take that distance off the level base once per level
// (mvx_ref_bias_bytes): no term of the sum is ever negative.
// Reach: a level's floored width trails its block grid by at most 3 samples (4:2:0: w' = floor(w / 4) * 2 >= w / 2 - 1.5 per level, the grid
// halves exactly or rounds down), so a clipped vector reaches 4 samples / rows outside at most; the 8-bit row passes start a lane's sixteen
// bytes up to 8 bytes early.  8 rows and 16 samples cover both with room, keep copy selection (offset mod 4) and 16-byte piece alignment.
#pragma once

#if defined(__HIPCC__)
#define MVX_AD_HD __host__ __device__ __forceinline__
#else
#define MVX_AD_HD static inline
#endif

#ifndef MVX_REF_BIAS_ROWS // (0 / 0 restates the arithmetic before the bias: the audit is built that way once, to show what it was)
#define MVX_REF_BIAS_ROWS 8
#endif
#ifndef MVX_REF_BIAS_COLS
#define MVX_REF_BIAS_COLS 16
#endif
static_assert(MVX_REF_BIAS_COLS % 16 == 0 && MVX_REF_BIAS_ROWS >= 0, "the bias keeps a piece's 16-byte alignment and the shifted copy a sample is read from");

// bytes between a level base and the base the 32-bit offsets of a plane with this pitch count from (a multiple of 16: pitches are)
MVX_AD_HD long long mvx_ref_bias_bytes(long long pitch, int bps) { return MVX_REF_BIAS_ROWS * pitch + (long long)MVX_REF_BIAS_COLS * bps; }

// With shadow copies the block at sample position x is read from copy k = x % (4 / BPS), where it starts at a dword-aligned
// address (copy k = the plane shifted left by k samples): same samples, ~3.7x cheaper for the CU's texture path.
template <int BPS> MVX_AD_HD unsigned mvx_shadow_off(unsigned off, unsigned shadow) {
    if (!shadow) return off;
    const unsigned k = BPS == 2 ? (off >> 1) & 1u : off & 3u;
    return (off & ~3u) + k * shadow;
}

// byte offset of sub-pel position (ax, ay) -- in units of 1 / pel sample, already counted from the moved origin -- inside a level's plane set.
// (The bias as ONE constant added to the plain offset -- correct modulo 2^32 -- was built and compared: it costs the kernels more registers than
// the moved origin, two lean builds an occupancy step: profiles/small_geometry_isa.txt.)
template <int BPS> MVX_AD_HD unsigned mvx_subpel_off32(int ax, int ay, int pel, int logPel, unsigned pstride, unsigned pitch) {
    const int m = pel - 1;
    const unsigned idx = (unsigned)((ax & m) | ((ay & m) << logPel));
    return idx * pstride + (unsigned)(ay >> logPel) * pitch + (unsigned)(ax >> logPel) * BPS;
}
// the luma block at (x0, y0) displaced by (vx, vy)  (PlaneOfBlocks.cpp:35-101, MVFrame.cpp:1707-1729)
template <int BPS> MVX_AD_HD unsigned mvx_luma_off32(int x0, int y0, int vx, int vy, int pel, int logPel, unsigned pstride, unsigned pitch) {
    return mvx_subpel_off32<BPS>(((x0 + MVX_REF_BIAS_COLS) << logPel) + vx, ((y0 + MVX_REF_BIAS_ROWS) << logPel) + vy, pel, logPel, pstride, pitch);
}
// the chroma block at (cx0, cy0) of the U (== V) plane; the vector is scaled towards zero's far side as the reference does (:836-839).
// In the UV-interleaved plane the offset is twice this (always dword-aligned), and so is the distance taken off its base.
template <int BPS> MVX_AD_HD unsigned mvx_chroma_off32(int cx0, int cy0, int vx, int vy, int lxr, int lyr, int pel, int logPel, unsigned pstride, unsigned pitch) {
    const int xbias = (vx < 0) ? ((1 << lxr) - 1) : 0, ybias = (vy < 0) ? ((1 << lyr) - 1) : 0;
    return mvx_subpel_off32<BPS>(((cx0 + MVX_REF_BIAS_COLS) << logPel) + ((vx + xbias) >> lxr), ((cy0 + MVX_REF_BIAS_ROWS) << logPel) + ((vy + ybias) >> lyr), pel, logPel, pstride, pitch);
}

// a lane's piece: `row` rows below and `xb` bytes right of the block's first sample / the distance a running offset advances by `rows` rows
MVX_AD_HD unsigned mvx_piece_off32(unsigned off, int row, unsigned pitch, int xb) { return off + (unsigned)row * pitch + (unsigned)xb; }
MVX_AD_HD unsigned mvx_rows_step32(int rows, unsigned pitch) { return (unsigned)rows * pitch; }
