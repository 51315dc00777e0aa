// mvx_dct_block.h -- the arithmetic of the dct = 1..4 cost modes (DCTFFTW.cpp:30-54, :135-208; PlaneOfBlocks.cpp:117-163), ONE text
// for the device (mvx_analyse_kernel.h, mvx_analyse_fdct.hip) and for the host (tests/dct_emu.cpp): what mvx_depan_fft_core.h is to
// mvx_depan_fft.hip.  Everything a result depends on is in here; who computes which coefficient (lanes on the device, plain loops on
// the host) is not arithmetic.
//
// Transform.  The reference runs fftwf_plan_r2r_2d(sizey, sizex, REDFT10, REDFT10): the unnormalised 2-D DCT-II,
//     Y[ky][kx] = sum_y sum_x  s[y][x] * 2 cos(pi (y + 1/2) ky / BH) * 2 cos(pi (x + 1/2) kx / BW).
// Here it is a direct separable float32 sum with a FIXED order:
//     row pass     R[y][kx]  = ((0 + s[y][0] * Cx[0][kx]) + s[y][1] * Cx[1][kx]) + ...       x ascending
//     column pass  Y[ky][kx] = ((0 + R[0][kx] * Cy[ky][0]) + R[1][kx] * Cy[ky][1]) + ...     y ascending
// every product rounded to float32, then every sum rounded to float32 (round to nearest even): NO fused multiply-add, on either
// side -- both builds pass -ffp-contract=off, and nothing below would contract otherwise except the one line in mvx_dct_dot.
// Cx[x][kx] = float32(2 cos(pi (x + 1/2) kx / BW)) and Cy[ky][y] = float32(2 cos(pi (y + 1/2) ky / BH)) are computed on the host in
// double and rounded once (mvx_dct_host.h).  Samples are integers below 2^16: exact in float32.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MVX_DCT_HD __host__ __device__ __forceinline__
#else
#define MVX_DCT_HD static inline
#endif

// sum_i x[i * xs] * c[i * cs], i ascending, product and sum rounded separately
template <typename XP, typename CP> MVX_DCT_HD float mvx_dct_dot(XP x, int xs, CP c, int cs, int n) {
    float acc = 0.0f;
    for (int i = 0; i < n; i++) {
        const float p = x[i * xs] * c[i * cs];
        acc = acc + p;
    }
    return acc;
}
// A: the block's samples as floats, row-major [bh][bw]; cxT: Cx[x][kx], row-major [bw][bw]
template <typename AP, typename CP> MVX_DCT_HD float mvx_dct_row(AP A, int y, int kx, int bw, CP cxT) { return mvx_dct_dot(A + y * bw, 1, cxT + kx, bw, bw); }
// B: the row pass's results [bh][bw]; cy: Cy[ky][y], row-major [bh][bh]
template <typename BP, typename CP> MVX_DCT_HD float mvx_dct_col(BP B, int ky, int kx, int bw, int bh, CP cy) { return mvx_dct_dot(B + kx, bw, cy + ky * bh, 1, bh); }

// Float2Pixels_C (DCTFFTW.cpp:30-54): every coefficient times sqrt(2)/2, rounded to nearest even, shifted arithmetically by dctshift,
// biased by half the range and clamped; element 0 (DC) is then overwritten with the same expression on f / 2 and dctshift + 2.
// |Y| <= 4 * 1024 * 65535 < 2^31 for the blocks this runs on (up to 32x32), so the conversion to int never overflows.
MVX_DCT_HD int mvx_dct_quant(float f, bool dc, int dctshift, int bits) {
    const float g = dc ? f * 0.5f : f * 0.70710678118654752440084436210485f;
    const int integ = (int)rintf(g);
    const int v = (integ >> (dc ? dctshift + 2 : dctshift)) + (1 << (bits - 1));
    const int mx = (1 << bits) - 1;
    return v < 0 ? 0 : (v > mx ? mx : v);
}

// pobLumaSAD's switch of modes 3 and 4 (PlaneOfBlocks.cpp:151, :159)
MVX_DCT_HD bool mvx_dct_luma_hit(int srcLuma, int refLuma) {
    const int d = srcLuma - refLuma;
    return (d < 0 ? -d : d) > ((srcLuma + refLuma) >> 5);
}
// does this candidate need the reference block's DCT at all?  (lumaHit is only read in modes 3 and 4)
MVX_DCT_HD bool mvx_dct_wanted(int mode, int weight16, bool lumaHit) { return mode == 1 || (mode == 2 && weight16 > 0) || ((mode == 3 || mode == 4) && lumaHit); }

// pobLumaSAD, modes 1..4 (PlaneOfBlocks.cpp:123-163).  sad: spatial SAD of the luma block; dctSad: sum |dctSrc - dctRef| over the block's
// quantised coefficients; dcAbs: |dctSrc[0] - dctRef[0]|.  64-bit where the reference's operands are int64_t.  dctSad and dcAbs are
// not read where mvx_dct_wanted() says no.
MVX_DCT_HD long long mvx_dct_cost(int mode, long long sad, unsigned dctSad, int dcAbs, int bw, bool lumaHit, int weight16) {
    const long long withDc = (long long)(dctSad + (unsigned)(dcAbs * 3)) * (long long)bw / 2; // "correct reduced DC component"
    const long long plain = (long long)dctSad * (long long)bw / 2;
    switch (mode) {
    case 1: return withDc;
    case 2: return weight16 > 0 ? (sad * (16 - weight16) + withDc * weight16) / 16 : sad;
    case 3: return lumaHit ? sad / 2 + plain / 2 : sad;
    case 4: return lumaHit ? sad / 4 + plain / 2 + plain / 4 : sad;
    default: return sad;
    }
}

#if defined(__HIPCC__)
// ---- one block by one 64-lane wave.  load(y, x) gives a sample; A and B are LDS scratch of bw * bh floats each, cxT / cy the basis tables
// in LDS; sink(t, q) receives the quantised coefficient t = ky * bw + kx (lane l owns t = l, l + 64, ...).  bw is a power of two.
// A wave's LDS operations execute in order; the fences keep the compiler from moving a pass's reads above the previous pass's writes.
#define MVX_DCT_LDS __attribute__((address_space(3)))
__device__ __forceinline__ void mvx_dct_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
template <typename LOAD, typename SINK>
__device__ __forceinline__ void mvx_dct_wave(int lane, int bw, int logBw, int bh, int bits, int dctshift, LOAD load, MVX_DCT_LDS float *A, MVX_DCT_LDS float *B,
                                             const MVX_DCT_LDS float *cxT, const MVX_DCT_LDS float *cy, SINK sink) {
    const int n = bw * bh;
    for (int t = lane; t < n; t += 64) A[t] = (float)load(t >> logBw, t & (bw - 1));
    mvx_dct_wave_sync();
    for (int t = lane; t < n; t += 64) B[t] = mvx_dct_row(A, t >> logBw, t & (bw - 1), bw, cxT);
    mvx_dct_wave_sync();
    for (int t = lane; t < n; t += 64) sink(t, mvx_dct_quant(mvx_dct_col(B, t >> logBw, t & (bw - 1), bw, bh, cy), t == 0, dctshift, bits));
    mvx_dct_wave_sync(); // A and B are free again
}
// LDS of the dct 1..4 builds behind a chain's ordinary regions: [dctSrc, 2 bytes per coefficient | A | B | cxT | cy]
__host__ __device__ inline int mvx_dct_lds_src(int bw, int bh) { return 0; }
__host__ __device__ inline int mvx_dct_lds_a(int bw, int bh) { return (2 * bw * bh + 15) & ~15; }
__host__ __device__ inline int mvx_dct_lds_b(int bw, int bh) { return mvx_dct_lds_a(bw, bh) + 4 * bw * bh; }
__host__ __device__ inline int mvx_dct_lds_cx(int bw, int bh) { return mvx_dct_lds_b(bw, bh) + 4 * bw * bh; }
__host__ __device__ inline int mvx_dct_lds_cy(int bw, int bh) { return mvx_dct_lds_cx(bw, bh) + 4 * bw * bw; }
__host__ __device__ inline int mvx_dct_lds_bytes(int bw, int bh) { return mvx_dct_lds_cy(bw, bh) + 4 * bh * bh; }
#endif
