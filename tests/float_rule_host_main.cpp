// Stand-alone host program for csrc/mvx_super_float_rule.h (test infrastructure; tests/test_float_host.py builds it at test time, with
// AddressSanitizer and UBSan where the compiler links them).  usage: float_rule_host_main SHARP ROWS N < ROWS*N float32 > 3*ROWS*N float32:
// the half-pel rule along every row, the sharp-0 diagonal of the rows taken as a plane, and the average of every row with the next (the last with
// the first).  Build with -ffp-contract=off, as the library is.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mvx_super_float_rule.h"

template <int SHARP> static void rows_half(const float *in, float *out, int rows, int n) {
    for (int r = 0; r < rows; r++) {
        const float *row = in + (size_t)r * n;
        for (int X = 0; X < n; X++) out[(size_t)r * n + X] = mvx_sf_half<SHARP>([&](int i) { return row[i]; }, X, n);
    }
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s SHARP ROWS N\n", argv[0]); return 2; }
    const int sharp = atoi(argv[1]), rows = atoi(argv[2]), n = atoi(argv[3]);
    if (sharp < 0 || sharp > 2 || rows < 1 || n < 1 || rows > 4096 || n > 4096) { fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t count = (size_t)rows * n;
    std::vector<float> in(count), out(3 * count);
    if (fread(in.data(), sizeof(float), count, stdin) != count) { fprintf(stderr, "short input\n"); return 2; }
    if (sharp == 0) rows_half<0>(in.data(), out.data(), rows, n);
    else if (sharp == 1) rows_half<1>(in.data(), out.data(), rows, n);
    else rows_half<2>(in.data(), out.data(), rows, n);
    for (int Y = 0; Y < rows; Y++)
        for (int X = 0; X < n; X++) {
            const bool lastRow = Y == rows - 1, lastCol = X == n - 1;
            const float a = in[(size_t)Y * n + X], b = lastCol ? 0.0f : in[(size_t)Y * n + X + 1];
            const float c = lastRow ? 0.0f : in[(size_t)(Y + 1) * n + X], d = (lastRow || lastCol) ? 0.0f : in[(size_t)(Y + 1) * n + X + 1];
            out[count + (size_t)Y * n + X] = mvx_sf_diagonal(a, b, c, d, lastRow, lastCol);
            out[2 * count + (size_t)Y * n + X] = mvx_sf_avg(a, in[(size_t)((Y + 1) % rows) * n + X]);
        }
    if (fwrite(out.data(), sizeof(float), 3 * count, stdout) != 3 * count) return 1;
    return 0;
}
