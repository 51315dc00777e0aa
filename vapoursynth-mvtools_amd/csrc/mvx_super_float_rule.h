// mvx_super_float_rule.h -- the per-sample arithmetic of the float Super (mvx_super_create_float), for device and host: the integer rules of
// mvx_super.hip (half_rule, the diagonal bilinear, super_avg_kernel) operation for operation in their order on float32, with the rounding
// term dropped, every shift a multiplication by the exact power of two, and no clamp: float samples may overshoot and float chroma is centred
// on 0.  The border rules are the integer ones.  Every operation is rounded on its own: build with -ffp-contract=off (build.py has it).
// tests/float_rule_host_main.cpp runs this header on the host against the numpy restatement (tests/super_float_ref.py).  Internal; not part
// of the ABI.
#pragma once

#if defined(__HIPCC__)
#define MVX_SF_HD __host__ __device__ __forceinline__
#else
#define MVX_SF_HD static inline
#endif

// horizontal / vertical half-pel sample at absolute padded coordinate X of a line of n samples; s(i) reads sample i as float
template <int SHARP, typename F> MVX_SF_HD float mvx_sf_half(F s, int X, int n) {
    if (X == n - 1) return s(X);
    if (SHARP == 0) return (s(X) + s(X + 1)) * 0.5f;
    if (SHARP == 1) {
        if (X < 1 || X >= n - 3) return (s(X) + s(X + 1)) * 0.5f;
        return ((s(X) + s(X + 1)) * 9.0f - (s(X - 1) + s(X + 2))) * 0.0625f;
    }
    if (X < 2 || X >= n - 4) return (s(X) + s(X + 1)) * 0.5f;
    float m0 = s(X - 2), m1 = s(X - 1), m2 = s(X), m3 = s(X + 1), m4 = s(X + 2), m5 = s(X + 3);
    m2 = (m2 + m3) * 4.0f; m2 -= (m1 + m4); m2 *= 5.0f; m0 = (m0 + m5) + m2;
    return m0 * 0.03125f;
}

// the diagonal plane of sharp 0 at (X, Y): a = (X, Y), b = (X + 1, Y), c = (X, Y + 1), d = (X + 1, Y + 1); samples past the last row / column are not used
MVX_SF_HD float mvx_sf_diagonal(float a, float b, float c, float d, bool lastRow, bool lastCol) {
    if (!lastRow) return !lastCol ? (((a + b) + c) + d) * 0.25f : (a + c) * 0.5f;
    return !lastCol ? (a + b) * 0.5f : a;
}

// an averaged plane of pel 4
MVX_SF_HD float mvx_sf_avg(float a, float b) { return (a + b) * 0.5f; }
