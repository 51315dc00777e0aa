// depan_show_emu.cpp -- test infrastructure: the text of DepanEstimate's show passes (csrc/mvx_depan_fft_core.h: the two inverse passes with every
// row of the surface kept, de_minmax, de_paint) compiled for the host, workgroup by workgroup in launch order, for tests/test_gpu_depan_show.py.
//   depan_show_emu IN OUT
// IN : 12 ints (winx winy wleft wleft2 wtop windows dxmax dymax bits16 pitch rows pixel_max), then the luma planes of prev and cur, pitch * rows bytes each
// OUT: per window the surface (winy * winx floats), then the plane of cur with the windows painted (pitch * rows bytes)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mvx_depan_fft_core.h"

static int ilog2(int i) { int r = 0; while (i > 1) { i /= 2; r++; } return r; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[12];
    if (fread(hd, 4, 12, f) != 12) return 2;
    DEParams P;
    memset(&P, 0, sizeof(P));
    P.winx = hd[0]; P.winy = hd[1]; P.wleft[0] = hd[2]; P.wleft[1] = hd[3]; P.wtop = hd[4]; P.nwin = hd[5]; P.dxmax = hd[6]; P.dymax = hd[7];
    P.bits16 = hd[8]; P.pitch = hd[9];
    const int rows = hd[10], pixel_max = hd[11];
    P.nx = P.winx / 2 + 1; P.lgx = ilog2(P.winx); P.lgy = ilog2(P.winy);
    P.cx = de_batch(P.winx); P.lgcx = ilog2(P.cx); P.cy = de_batch(P.winy); P.lgcy = ilog2(P.cy);
    P.nrows = P.winy; P.jshift = 0;   // every row
    std::vector<unsigned char> plane[2];
    for (int k = 0; k < 2; k++) {
        plane[k].resize((size_t)P.pitch * rows);
        if (fread(plane[k].data(), 1, plane[k].size(), f) != plane[k].size()) return 2;
    }
    fclose(f);
    std::vector<DEComplex> twx(P.winx / 2), twy(P.winy / 2);
    de_twiddles(twx.data(), P.winx);
    de_twiddles(twy.data(), P.winy);
    const size_t one = (size_t)P.winy * P.nx;
    std::vector<DEComplex> spec[2];
    std::vector<float> re(DE_LDS_COMPLEX), im(DE_LDS_COMPLEX);
    const int rgroups = (P.winy / 2 + P.cx - 1) / P.cx, cgroups = (P.nx + P.cy - 1) / P.cy;
    for (int k = 0; k < 2; k++) {
        spec[k].resize(one * P.nwin);
        for (int w = 0; w < P.nwin; w++) {
            for (int g = 0; g < rgroups; g++) de_rows_forward(P, plane[k].data(), w, g, spec[k].data() + one * w, twx.data(), re.data(), im.data());
            for (int g = 0; g < cgroups; g++) de_cols_forward(P, g, spec[k].data() + one * w, twy.data(), re.data(), im.data());
        }
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    std::vector<DEComplex> half((size_t)P.winy * P.nx);
    std::vector<float> corr((size_t)P.winy * P.winx);
    std::vector<float> lmin(DE_THREADS), lmax(DE_THREADS);
    const int sgroups = de_show_groups(P.winx * P.winy);
    std::vector<float> partial(2 * sgroups);
    for (int w = 0; w < P.nwin; w++) {
        for (int g = 0; g < cgroups; g++) de_cols_correlate(P, g, spec[1].data() + one * w, spec[0].data() + one * w, half.data(), twy.data(), re.data(), im.data());
        for (int g = 0; g < rgroups; g++) de_rows_inverse(P, g, half.data(), corr.data(), twx.data(), re.data(), im.data());
        for (int g = 0; g < sgroups; g++) de_minmax(P, corr.data(), g, sgroups, partial.data(), lmin.data(), lmax.data());
        for (int g = 0; g < sgroups; g++) de_paint(P, corr.data(), partial.data(), g, sgroups, plane[1].data(), w, pixel_max, lmin.data(), lmax.data());
        fwrite(corr.data(), sizeof(float), corr.size(), o);
    }
    fwrite(plane[1].data(), 1, plane[1].size(), o);
    fclose(o);
    return 0;
}
