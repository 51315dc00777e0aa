// mvx_dct_host.h -- host part of the dct = 1..4 cost modes: the basis tables and dctshift (dctInit, DCTFFTW.cpp:135-149).  Plain C++,
// no device code: the library includes it at create, tests/dct_emu.cpp and tests/dct_host_main.cpp include it for the host.
#pragma once
#include <math.h>
#include <vector>

// the largest block the dct 1..4 builds take (their per-wave transform keeps two float copies of the block in LDS)
#define MVX_DCT_MAX_SAMPLES 1024

// dctshift = ceil(log2(sizex * sizey)), as the reference's loop finds it
inline int mvx_dct_shift(int bw, int bh) {
    int shift = 0;
    for (long long cur = 1; cur < (long long)bw * bh; cur <<= 1) shift++;
    return shift;
}

// [ Cx[x][kx], bw * bw | Cy[ky][y], bh * bh ]: 2 cos(pi (i + 1/2) k / n) in double, rounded once to float.  Cx is stored sample-major
// (the row pass of a wave reads it with kx across the lanes), Cy coefficient-major.
inline std::vector<float> mvx_dct_tables(int bw, int bh) {
    const double pi = 3.14159265358979323846;
    std::vector<float> t((size_t)bw * bw + (size_t)bh * bh);
    for (int x = 0; x < bw; x++)
        for (int k = 0; k < bw; k++) t[(size_t)x * bw + k] = (float)(2.0 * cos(pi * (x + 0.5) * k / bw));
    float *cy = t.data() + (size_t)bw * bw;
    for (int k = 0; k < bh; k++)
        for (int y = 0; y < bh; y++) cy[(size_t)k * bh + y] = (float)(2.0 * cos(pi * (y + 0.5) * k / bh));
    return t;
}
