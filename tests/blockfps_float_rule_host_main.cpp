// Stand-alone host program for csrc/mvx_blockfps_float_rule.h (test infrastructure; tests/test_blockfps_float_host.py builds it at test time, with
// AddressSanitizer and UBSan where the compiler links them).  usage: blockfps_float_rule_host_main MODE N < input > 3 * N float32.
// input: four arrays of N float32 (sVal, rVal, b, fw), then eight arrays of N int32 (mF, mB, mO, time256, four window weights).
// output: the mode's value; the time blend of rVal over sVal (the strips and the blended fallback); and the overlap rule over four terms -- the
// value, sVal, rVal and b with the four weights in that order, divided by the weights' sum.  Build with -ffp-contract=off, as the library is.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mvx_blockfps_float_rule.h"

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s MODE N\n", argv[0]); return 2; }
    const int mode = atoi(argv[1]), n = atoi(argv[2]);
    if (mode < 0 || mode > 8 || n < 1 || n > (1 << 22)) { fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t N = (size_t)n;
    std::vector<float> f(4 * N), out(3 * N);
    std::vector<int32_t> k(8 * N);
    if (fread(f.data(), sizeof(float), 4 * N, stdin) != 4 * N || fread(k.data(), sizeof(int32_t), 8 * N, stdin) != 8 * N) { fprintf(stderr, "short input\n"); return 2; }
    for (size_t i = 0; i < N; i++) {
        const float s = f[i], r = f[N + i], b = f[2 * N + i], fw = f[3 * N + i];
        const int mF = k[i], mB = k[N + i], mO = k[2 * N + i], t = k[3 * N + i];
        const int32_t *w = &k[4 * N + i];
        const float v = mvx_bff_value(mode, t, s, r, b, fw, mF, mB, mO);
        out[i] = v;
        out[N + i] = mvx_bff_time(r, s, t);
        const float term[4] = { v, s, r, b };
        float acc = 0.0f;
        int wsum = 0;
        for (int j = 0; j < 4; j++) { acc = mvx_bff_add(acc, term[j], w[j * N]); wsum += w[j * N]; }
        out[2 * N + i] = mvx_bff_out(acc, wsum);
    }
    if (fwrite(out.data(), sizeof(float), 3 * N, stdout) != 3 * N) return 1;
    return 0;
}
