// Stand-alone host program for csrc/mvx_flow_float_rule.h (test infrastructure; tests/test_flow_float_host.py builds it at test time, with
// AddressSanitizer and UBSan where the compiler links them).  usage: flow_float_rule_host_main N < input > 4 * N float32.
// input: six arrays of N float32 (dF, dB, dF0, dB0, dFF, dBB), then three arrays of N int32 (mF, mB, time256).
// output: Simple, Regular, Extra, and the blend of dB0 (right) over dF0 (left).  Build with -ffp-contract=off, as the library is.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mvx_flow_float_rule.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s N\n", argv[0]); return 2; }
    const int n = atoi(argv[1]);
    if (n < 1 || n > (1 << 22)) { fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t N = (size_t)n;
    std::vector<float> f(6 * N), out(4 * N);
    std::vector<int32_t> k(3 * N);
    if (fread(f.data(), sizeof(float), 6 * N, stdin) != 6 * N || fread(k.data(), sizeof(int32_t), 3 * N, stdin) != 3 * N) { fprintf(stderr, "short input\n"); return 2; }
    for (size_t i = 0; i < N; i++) {
        const float dF = f[i], dB = f[N + i], dF0 = f[2 * N + i], dB0 = f[3 * N + i], dFF = f[4 * N + i], dBB = f[5 * N + i];
        const int mF = k[i], mB = k[N + i], t = k[2 * N + i];
        out[i] = mvx_flf_simple(t, dF, dB, mF, mB);
        out[N + i] = mvx_flf_regular(t, dF, dB, dF0, dB0, mF, mB);
        out[2 * N + i] = mvx_flf_extra(t, dF, dB, dFF, dBB, mF, mB);
        out[3 * N + i] = mvx_flf_blend(t, dF0, dB0);
    }
    if (fwrite(out.data(), sizeof(float), 4 * N, stdout) != 4 * N) return 1;
    return 0;
}
