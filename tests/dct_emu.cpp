// The arithmetic of the dct 1..4 cost modes (csrc/mvx_dct_block.h, csrc/mvx_dct_host.h) compiled for the host: the exact yardstick of
// the device path.  Built by tests/dct_oracle.py with g++ -ffp-contract=off into a shared library; TEST INFRASTRUCTURE ONLY.
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

#include "mvx_dct_block.h"
#include "mvx_dct_host.h"

namespace {
struct Tables { int bw = 0, bh = 0; std::vector<float> t; };
const float *tables(int bw, int bh) {
    static thread_local Tables T;
    if (T.bw != bw || T.bh != bh) { T.t = mvx_dct_tables(bw, bh); T.bw = bw; T.bh = bh; }
    return T.t.data();
}
inline int sample(const void *p, ptrdiff_t pitch, int bits, int y, int x) {
    const uint8_t *row = (const uint8_t *)p + (ptrdiff_t)y * pitch;
    return bits <= 8 ? (int)row[x] : (int)((const uint16_t *)row)[x];
}
// the raw coefficients Y[ky][kx], in the order and rounding mvx_dct_block.h fixes
void coeffs(const void *src, ptrdiff_t pitch, int bw, int bh, int bits, float *Y) {
    const float *cxT = tables(bw, bh), *cy = cxT + (size_t)bw * bw;
    std::vector<float> A((size_t)bw * bh), B((size_t)bw * bh);
    for (int y = 0; y < bh; y++)
        for (int x = 0; x < bw; x++) A[(size_t)y * bw + x] = (float)sample(src, pitch, bits, y, x);
    for (int y = 0; y < bh; y++)
        for (int k = 0; k < bw; k++) B[(size_t)y * bw + k] = mvx_dct_row(A.data(), y, k, bw, cxT);
    for (int ky = 0; ky < bh; ky++)
        for (int kx = 0; kx < bw; kx++) Y[(size_t)ky * bw + kx] = mvx_dct_col(B.data(), ky, kx, bw, bh, cy);
}
#ifdef DCT_EMU_F64
// -DDCT_EMU_F64: the same interface driven by a float64 transform (separable, cosines from libm) and the quantiser restated on doubles.  Only
// tools/dct_precision.py builds it, to report how many vectors the float32 arithmetic moves; no test holds the library to it.
void bytes(const void *src, ptrdiff_t pitch, int bw, int bh, int bits, int *q) {
    const double pi = 3.14159265358979323846;
    std::vector<double> R((size_t)bw * bh), Y((size_t)bw * bh);
    for (int y = 0; y < bh; y++)
        for (int k = 0; k < bw; k++) {
            double acc = 0;
            for (int x = 0; x < bw; x++) acc += sample(src, pitch, bits, y, x) * 2.0 * cos(pi * (x + 0.5) * k / bw);
            R[(size_t)y * bw + k] = acc;
        }
    const int shift = mvx_dct_shift(bw, bh), half = 1 << (bits - 1), mx = (1 << bits) - 1;
    for (int ky = 0; ky < bh; ky++)
        for (int kx = 0; kx < bw; kx++) {
            double acc = 0;
            for (int y = 0; y < bh; y++) acc += R[(size_t)y * bw + kx] * 2.0 * cos(pi * (y + 0.5) * ky / bh);
            const bool dc = ky == 0 && kx == 0;
            const long long integ = (long long)rint(acc * (dc ? 0.5 : (double)0.70710678118654752440084436210485f));
            const long long v = (integ >> (dc ? shift + 2 : shift)) + half;
            q[(size_t)ky * bw + kx] = (int)(v < 0 ? 0 : (v > mx ? mx : v));
        }
}
#else
void bytes(const void *src, ptrdiff_t pitch, int bw, int bh, int bits, int *q) {
    std::vector<float> Y((size_t)bw * bh);
    coeffs(src, pitch, bw, bh, bits, Y.data());
    const int shift = mvx_dct_shift(bw, bh);
    for (int t = 0; t < bw * bh; t++) q[t] = mvx_dct_quant(Y[t], t == 0, shift, bits);
}
#endif
}

extern "C" {
// raw float coefficients of one block (bw * bh floats)
void dct_emu_coeffs(const void *src, ptrdiff_t pitch, int bw, int bh, int bits, float *out) { coeffs(src, pitch, bw, bh, bits, out); }
// quantised coefficients of one block in the sample type (bw * bh samples, densely packed)
void dct_emu_block(const void *src, ptrdiff_t pitch, int bw, int bh, int bits, void *out) {
    std::vector<int> q((size_t)bw * bh);
    bytes(src, pitch, bw, bh, bits, q.data());
    for (int t = 0; t < bw * bh; t++) {
        if (bits <= 8) ((uint8_t *)out)[t] = (uint8_t)q[t];
        else ((uint16_t *)out)[t] = (uint16_t)q[t];
    }
}
// the quantiser alone (the float64 yardstick's bytes go through the same text)
int dct_emu_quant(float f, int dc, int shift, int bits) { return mvx_dct_quant(f, dc != 0, shift, bits); }
// the cost formula alone
long long dct_emu_cost_formula(int mode, long long sad, unsigned dctSad, int dcAbs, int bw, int lumaHit, int weight16) {
    return mvx_dct_cost(mode, sad, dctSad, dcAbs, bw, lumaHit != 0, weight16);
}
// pobLumaSAD for dct 1..4 of one candidate: spatial SAD, the reference block's luma sum where the mode reads it, both blocks' DCT where
// the mode wants it
long long dct_emu_luma_cost(const void *src, ptrdiff_t spitch, const void *ref, ptrdiff_t rpitch, int bw, int bh, int bits, int mode, int srcLuma,
                            int weight16) {
    long long sad = 0;
    int refLuma = 0;
    for (int y = 0; y < bh; y++)
        for (int x = 0; x < bw; x++) {
            const int s = sample(src, spitch, bits, y, x), r = sample(ref, rpitch, bits, y, x);
            sad += abs(s - r);
            refLuma += r;
        }
    const bool hit = (mode == 3 || mode == 4) && mvx_dct_luma_hit(srcLuma, refLuma);
    if (!mvx_dct_wanted(mode, weight16, hit)) return mvx_dct_cost(mode, sad, 0, 0, bw, hit, weight16);
    std::vector<int> a((size_t)bw * bh), b((size_t)bw * bh);
    bytes(src, spitch, bw, bh, bits, a.data());
    bytes(ref, rpitch, bw, bh, bits, b.data());
    unsigned d = 0;
    for (int t = 0; t < bw * bh; t++) d += (unsigned)abs(a[t] - b[t]);
    return mvx_dct_cost(mode, sad, d, abs(a[0] - b[0]), bw, hit, weight16);
}
}
