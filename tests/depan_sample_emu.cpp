// depan_sample_emu.cpp -- test infrastructure: DepanCompensate's per-sample arithmetic (csrc/mvx_depan_sample.h, the text the GPU kernel
// runs per thread) compiled for the host, one plane per call, so that tests/test_depan_ref.py can hold it to the restatement without a GPU.
#include <string.h>
#include <vector>
#include "mvx_depan_sample.h"

template <typename T> static void plane(const DCPlane &P, const DCCommon &C, int sub) {
    for (int h = 0; h < P.H; h++)
        for (int row = 0; row < P.W; row++)
            ((T *)(P.dst + (long long)h * P.dpitch))[row] = (T)(sub == 0 ? dc_nearest<T>(P, C, h, row) : sub == 1 ? dc_bilinear<T>(P, C, h, row) : dc_bicubic<T>(P, C, h, row));
}

extern "C" void depan_emu_plane(const unsigned char *src, long long spitch, int W, int H, int bps, int sub, int mirror, int pixel_max, int border, int blur,
                                const float *tr, unsigned char *dst, long long dpitch) {
    DCPlane P;
    memset(&P, 0, sizeof(P));
    P.src = src; P.dst = dst; P.spitch = spitch; P.dpitch = dpitch; P.W = W; P.H = H;
    P.dxc = tr[0]; P.dxx = tr[1]; P.dxy = tr[2]; P.dyc = tr[3]; P.dyx = tr[4]; P.dyy = tr[5];
    P.cls = (tr[2] == 0.0f && tr[4] == 0.0f && tr[1] == 1.0f && tr[5] == 1.0f) ? 0 : (tr[2] == 0.0f && tr[4] == 0.0f) ? 1 : 2;
    P.border = border; P.blur = blur; P.segs = (W + DC_SEG - 1) / DC_SEG;
    std::vector<float> chain((size_t)H * P.segs * 2);
    P.chain = chain.data();
    if (P.cls == 2 && sub < 2) for (int h = 0; h < H; h++) dc_chain_row(P, h);
    const DCCommon C = { mirror, pixel_max, 1 };
    if (bps == 1) plane<unsigned char>(P, C, sub); else plane<unsigned short>(P, C, sub);
}

#ifdef DEPAN_EMU_MAIN
// depan_sample_emu IN OUT -- IN: W H bps sub mirror pixel_max border blur as ints, six floats, the source plane without padding; OUT: the
// destination plane.  The source and destination are heap blocks of exactly the plane's size, so that a sanitizer sees any index outside them.
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int hd[8];
    float tr[6];
    if (!f || fread(hd, 4, 8, f) != 8 || fread(tr, 4, 6, f) != 6) return 2;
    const size_t n = (size_t)hd[0] * hd[1] * hd[2];
    std::vector<unsigned char> src(n), dst(n);
    if (fread(src.data(), 1, n, f) != n) return 2;
    fclose(f);
    depan_emu_plane(src.data(), (long long)hd[0] * hd[2], hd[0], hd[1], hd[2], hd[3], hd[4], hd[5], hd[6], hd[7], tr, dst.data(), (long long)hd[0] * hd[2]);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(dst.data(), 1, n, f) != n) return 2;
    fclose(f);
    return 0;
}
#endif
