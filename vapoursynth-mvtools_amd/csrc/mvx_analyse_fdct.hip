// The dct = 1..4 builds of the generic search kernel and of the Recalculate kernel (the float block DCT of mvx_dct_block.h as luma cost),
// and the test entry that runs the device transform and quantiser alone.  A translation unit of their own: their code must not reach
// the register allocation of any other search kernel (mvx_analyse_kernel.h: Geo).
#include "mvx_analyse_kernel.h"

int mvx_analyse_launch_fdct(const AParams &P, const ALaunch &L) {
    if (L.cpw == 4) return P.bps == 1 ? launch_analyse_kernel<1, GeoAnyFdct, 1, 4>(L) : launch_analyse_kernel<2, GeoAnyFdct, 1, 4>(L);
    return P.bps == 1 ? launch_analyse_kernel<1, GeoAnyFdct>(L) : launch_analyse_kernel<2, GeoAnyFdct>(L);
}

int mvx_recalc_launch_fdct(const AParams &P, const RLaunch &L) {
    if (P.bps == 1) hipLaunchKernelGGL((recalc_fdct_kernel<1>), dim3(L.nBlk, L.njobs), dim3(64), L.ldsBytes, L.st, L.dP, L.dR, L.dJobs, L.ldsRow, L.ldsHist, L.histBins);
    else hipLaunchKernelGGL((recalc_fdct_kernel<2>), dim3(L.nBlk, L.njobs), dim3(64), L.ldsBytes, L.st, L.dP, L.dR, L.dJobs, L.ldsRow, L.ldsHist, L.histBins);
    return MVX_OK;
}

// mvx_analyse_dct_blocks: one wave per block; LDS = [A | B | cxT | cy]
template <int BPS>
__global__ __launch_bounds__(64) void dct_blocks_kernel(const unsigned char *plane, long long pitch, const int *xs, const int *ys, unsigned char *out, const float *tab, int bw,
                                                         int bh, int bits, int dctshift) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int l = threadIdx.x, n = bw * bh, b = blockIdx.x;
    MVX_DCT_LDS float *A = (MVX_DCT_LDS float *)(lds_u8 *)smem, *B = A + n, *cxT = B + n, *cy = cxT + bw * bw;
    for (int i = l; i < bw * bw + bh * bh; i += 64) cxT[i] = tab[i];
    mvx_dct_wave_sync();
    const unsigned char *blk = plane + (long long)ys[b] * pitch + (long long)xs[b] * BPS;
    unsigned char *o = out + (size_t)b * n * BPS;
    mvx_dct_wave(l, bw, 31 - __builtin_clz((unsigned)bw), bh, bits, dctshift,
                 [=](int y, int x) { return BPS == 1 ? (int)blk[(long long)y * pitch + x] : (int)*(const uh1 *)(blk + (long long)y * pitch + 2 * x); }, A, B, cxT, cy,
                 [=](int t, int q) { if (BPS == 1) o[t] = (unsigned char)q; else ((unsigned short *)o)[t] = (unsigned short)q; });
}

int mvx_dct_blocks_launch(const AParams &P, const void *plane, long long pitch, int n, const int *dXs, const int *dYs, void *out, hipStream_t st) {
    const int lds = 4 * (2 * P.blkX * P.blkY + P.blkX * P.blkX + P.blkY * P.blkY);
    if (P.bps == 1) hipLaunchKernelGGL((dct_blocks_kernel<1>), dim3(n), dim3(64), lds, st, (const unsigned char *)plane, pitch, dXs, dYs, (unsigned char *)out, P.dctTab, P.blkX, P.blkY, P.bits, P.dctShift);
    else hipLaunchKernelGGL((dct_blocks_kernel<2>), dim3(n), dim3(64), lds, st, (const unsigned char *)plane, pitch, dXs, dYs, (unsigned char *)out, P.dctTab, P.blkX, P.blkY, P.bits, P.dctShift);
    HIP_CHECK(hipGetLastError());
    return MVX_OK;
}
