// Stand-alone driver of csrc/mvx_dct_host.h (and, through it, of the host side of csrc/mvx_dct_block.h), built by tests/test_dct_host.py with
// -fsanitize=address,undefined and run as its own program: the tables and dctshift of every legal block shape, and whole blocks at the ends of the
// sample range through the transform, the quantiser and the cost formulas (the int conversion, the shifts and the 64-bit products at their largest).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mvx_dct_block.h"
#include "mvx_dct_host.h"

static int fail(const char *what, int a, int b) {
    fprintf(stderr, "dct_host_main: %s (%d, %d)\n", what, a, b);
    return 1;
}

int main() {
    static const int shapes[][3] = { { 4, 4, 4 }, { 8, 4, 5 }, { 8, 8, 6 }, { 16, 2, 5 }, { 16, 8, 7 }, { 16, 16, 8 }, { 32, 16, 9 }, { 32, 32, 10 } };
    for (const auto &s : shapes) {
        const int bw = s[0], bh = s[1];
        if (bw * bh > MVX_DCT_MAX_SAMPLES) return fail("shape above the limit", bw, bh);
        if (mvx_dct_shift(bw, bh) != s[2]) return fail("dctshift", bw, bh);
        const std::vector<float> t = mvx_dct_tables(bw, bh);
        if ((int)t.size() != bw * bw + bh * bh) return fail("table size", bw, bh);
        const float *cxT = t.data(), *cy = cxT + bw * bw;
        for (int x = 0; x < bw; x++)
            if (cxT[x * bw] != 2.0f) return fail("Cx[x][0] != 2", bw, x);
        for (int y = 0; y < bh; y++)
            if (cy[y] != 2.0f) return fail("Cy[0][y] != 2", bh, y);
        for (size_t i = 0; i < t.size(); i++)
            if (!(t[i] >= -2.0f && t[i] <= 2.0f)) return fail("table entry out of range", bw, (int)i);
        for (int bits : { 8, 10, 16 }) {
            const int mx = (1 << bits) - 1, shift = mvx_dct_shift(bw, bh), n = bw * bh;
            for (int kind = 0; kind < 3; kind++) { // all zero, all max, checker
                std::vector<float> A(n), B(n);
                for (int i = 0; i < n; i++) A[i] = kind == 0 ? 0.0f : kind == 1 ? (float)mx : (float)((((i % bw) + (i / bw)) & 1) * mx);
                for (int y = 0; y < bh; y++)
                    for (int k = 0; k < bw; k++) B[y * bw + k] = mvx_dct_row(A.data(), y, k, bw, cxT);
                long long sum = 0;
                int q0 = 0;
                for (int ky = 0; ky < bh; ky++)
                    for (int kx = 0; kx < bw; kx++) {
                        const int q = mvx_dct_quant(mvx_dct_col(B.data(), ky, kx, bw, bh, cy), ky == 0 && kx == 0, shift, bits);
                        if (q < 0 || q > mx) return fail("byte out of range", bw, bh);
                        if (ky == 0 && kx == 0) q0 = q;
                        sum += q;
                    }
                // a flat block: every AC byte is half the range; the DC byte is half + (level * n rounded) >> (shift + 2), clamped
                const int half = 1 << (bits - 1);
                if (kind == 0 && (q0 != half || sum != (long long)half * n)) return fail("zero block", bw, bh);
                if (kind == 1 && q0 != (((int)(2LL * mx * n) >> (shift + 2)) + half > mx ? mx : ((int)(2LL * mx * n) >> (shift + 2)) + half)) return fail("max block DC", q0, bits);
            }
        }
    }
    // quantiser at the ends of its input range (|Y| <= 4 * 1024 * 65535) and the cost formulas at their largest operands
    const float big = 4.0f * 1024.0f * 65535.0f;
    if (mvx_dct_quant(big, false, 10, 16) != 65535 || mvx_dct_quant(-big, false, 10, 16) != 0 || mvx_dct_quant(big, true, 10, 16) != 65535 || mvx_dct_quant(-big, true, 10, 16) != 0)
        return fail("quantiser clamp", 0, 0);
    if (mvx_dct_quant(-1.0f, false, 4, 8) != 127 || mvx_dct_quant(-0.5f, false, 4, 8) != 128) return fail("arithmetic shift of a negative value", 0, 0);
    const unsigned dmax = 1024u * 65535u;
    if (mvx_dct_cost(1, 0, dmax, 65535, 32, false, 0) != ((long long)dmax + 3LL * 65535) * 16) return fail("mode 1 at the largest operands", 0, 0);
    if (mvx_dct_cost(2, dmax, dmax, 65535, 32, false, 16) != ((long long)dmax + 3LL * 65535) * 16) return fail("mode 2, weight 16", 0, 0);
    if (mvx_dct_cost(2, 12345, dmax, 65535, 32, false, 0) != 12345) return fail("mode 2, weight 0", 0, 0);
    if (mvx_dct_cost(3, 1001, 11, 5, 8, true, 0) != 500 + 22 || mvx_dct_cost(3, 1001, 11, 5, 8, false, 0) != 1001) return fail("mode 3", 0, 0);
    if (mvx_dct_cost(4, 1001, 11, 5, 8, true, 0) != 250 + 22 + 11) return fail("mode 4", 0, 0);
    if (!mvx_dct_luma_hit(1000, 900) || mvx_dct_luma_hit(1000, 960) || !mvx_dct_wanted(1, 0, false) || mvx_dct_wanted(2, 0, false) || !mvx_dct_wanted(4, 0, true) || mvx_dct_wanted(3, 16, false))
        return fail("switches", 0, 0);
    printf("dct_host_main: ok\n");
    return 0;
}
