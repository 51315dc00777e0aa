// mvx_blockfps_float_rule.h -- the per-sample arithmetic of the float BlockFPS (mvx_blockfps_create_float), for device and host: RealResultBlock
// (MVBlockFPS.c:117-227), Blend (MaskFun.cpp:349-371) and the overlap sum on float32.  The time weights stay the integers t and 256 - t and the
// ">> 8" becomes a multiplication by the exact 1 / 256; the mask mixes divide by 255, the weights' own sum, where the reference has
// "(... + 255) >> 8"; the overlap sum is DegrainN-float's (acc = acc + v * win, then acc / wsum).  No rounding term, no clamp, no wrap: float
// samples may be negative or overshoot.  Every operation is rounded on its own: build with -ffp-contract=off (build.py has it).  Minimum and
// maximum are comparisons and selects, so that equal operands (and zeros of either sign) give the SECOND one on every compiler.
// tests/blockfps_float_rule_host_main.cpp runs this header on the host against the numpy restatement (tests/blockfps_float_ref.py).  Internal;
// not part of the ABI.
#pragma once

#if defined(__HIPCC__)
#define MVX_BFF_HD __host__ __device__ __forceinline__
#else
#define MVX_BFF_HD static inline
#endif

MVX_BFF_HD float mvx_bff_min(float a, float b) { return a < b ? a : b; }
MVX_BFF_HD float mvx_bff_max(float a, float b) { return a > b ? a : b; }
// med(a, b, c) = max(min(a, b), min(max(a, b), c))
MVX_BFF_HD float mvx_bff_med(float a, float b, float c) { return mvx_bff_max(mvx_bff_min(a, b), mvx_bff_min(mvx_bff_max(a, b), c)); }
// the value at time t (1..255 of 256) between `left` (weight 256 - t) and `right` (weight t)
MVX_BFF_HD float mvx_bff_time(float right, float left, int t) { return (right * (float)t + left * (float)(256 - t)) * 0.00390625f; }
// mix(m, p, q): p at mask 255, q at mask 0
MVX_BFF_HD float mvx_bff_mix(int m, float p, float q) { return ((float)m * p + (float)(255 - m) * q) / 255.0f; }

// one sample of a block.  sVal / rVal: the left / right frame at the output position; b: the fetch from the right frame along the backward
// vector; fw: the fetch from the left frame along the forward vector; mF, mB, mO: the upsized masks, 0..255 (0 where the mode reads none)
MVX_BFF_HD float mvx_bff_value(int mode, int t, float sVal, float rVal, float b, float fw, int mF, int mB, int mO) {
    switch (mode) {
    case 0: return mvx_bff_time(b, fw, t);
    case 1: return mvx_bff_med(rVal, sVal, mvx_bff_time(b, fw, t));
    case 2: return mvx_bff_med(mvx_bff_time(rVal, sVal, t), b, fw);
    case 3: case 6: return mvx_bff_time(mvx_bff_mix(mB, fw, b), mvx_bff_mix(mF, b, fw), t);
    case 4: case 7: {
        const float avg = mvx_bff_time(rVal, sVal, t), m = mvx_bff_time(mvx_bff_mix(mB, fw, b), mvx_bff_mix(mF, b, fw), t);
        return mvx_bff_mix(mO, avg, m);
    }
    default: return (float)mO / 255.0f;
    }
}

// overlapped blocks: one covering block's term, and the end
MVX_BFF_HD float mvx_bff_add(float acc, float v, int win) { return acc + v * (float)win; }
MVX_BFF_HD float mvx_bff_out(float acc, int wsum) { return acc / (float)wsum; }
