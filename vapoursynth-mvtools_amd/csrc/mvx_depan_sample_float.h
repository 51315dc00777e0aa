// mvx_depan_sample_float.h -- the warp of DepanCompensate and DepanStabilise for one output sample of a 32-bit float clip: what
// depan_warp_kernel<float, SUB, NSRC> of mvx_depan_warp.hip runs per thread.
//
// Positions are the integer path's, value for value: every function here is its namesake of mvx_depan_sample.h (dcf_nearest is dc_nearest, ...)
// with the same form, checkpoints, rowleft / hlow, kx / ky in 32nds, ix / iy in 256ths, sx / sy, mirror bits, blur runs, edge rows and
// columns, the NaN / 2^30 guard and the out-of-row border (divergences 2a-2c of mvtools_amd.h).  Only what a branch returns differs:
//   copies     move the sample's 32 bits (nearest, an unblurred mirror column, bicubic's edge columns, the bottom-row copies): a sample is
//              carried as uint32_t, so a NaN payload, a denormal or -0.0f arrives as it left.
//   border     0.0f luma, 0.5f chroma: DCPlane::border holds 0 or 1 (the value in halves) and -1 for a pass that leaves the sample alone.
//   blur run   the float32 sum from 0.0f in index order, divided by blurlen.
//   bilinear   top = (32 - kx) * a + kx * b, bot likewise on the row below, ((32 - ky) * top + ky * bot) * (1.0f / 1024), in all three forms.
//   bicubic    four row sums over dc_cub(ix, .), their column sum over dc_cub(iy, .), divided once by the product of the two coefficient
//              totals, in all three forms; no >> 22, no clamp.  The near-edge rows are dc_edge_double's expression in float32; the zoom
//              form's bottom row is (a + b) * 0.5f.
// Nothing is fused (build with -ffp-contract=off) and nothing is clamped.  A function returns whether it painted: a float sample may be
// negative, so DepanStabilise's selection cannot use the integer path's `v < 0`.
// A header without HIP, as mvx_depan_sample.h: tests/depan_float_emu.cpp compiles the same text for the host.
#pragma once
#include <stdint.h>
#include "mvx_depan_sample.h"

DC_FN float dcf_val(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }
DC_FN uint32_t dcf_bits(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }
DC_FN uint32_t dcf_px(const DCPlane &P, int y, int x) { return ((const uint32_t *)(P.src + (long long)y * P.spitch))[x]; }
DC_FN float dcf_pf(const DCPlane &P, int y, int x) { return dcf_val(dcf_px(P, y, x)); }

DC_FN bool dcf_border(const DCPlane &P, uint32_t &v) {
    if (P.border < 0) return false;
    v = dcf_bits(0.5f * (float)P.border);
    return true;
}
DC_FN bool dcf_copy(const DCPlane &P, int y, int x, uint32_t &v) { v = dcf_px(P, y, x); return true; }
// the mean of the run [lo, lo + blurlen) of row hlow
DC_FN bool dcf_run(const DCPlane &P, int hlow, int lo, int blurlen, uint32_t &v) {
    float smoothed = 0.0f;
    for (int i = lo; i < lo + blurlen; i++) smoothed += dcf_pf(P, hlow, i);
    v = dcf_bits(smoothed / (float)blurlen);
    return true;
}

DC_FN bool dcf_left(const DCPlane &P, int hlow, int rowleft, int blurmax, uint32_t &v) {
    if (-rowleft >= P.W) return dcf_border(P, v);
    if (blurmax > 0) {
        const int blurlen = dc_min(blurmax, -rowleft);
        return dcf_run(P, hlow, -rowleft - blurlen + 1, blurlen, v);
    }
    return dcf_copy(P, hlow, -rowleft, v);
}
DC_FN bool dcf_right(const DCPlane &P, int hlow, int rowleft, int blurmax, int add, uint32_t &v) {
    const int lo = P.W + P.W - rowleft - 2;
    if (lo < 0) return dcf_border(P, v);
    if (blurmax > 0) return dcf_run(P, hlow, lo, dc_min(blurmax, rowleft - P.W + add), v);
    return dcf_copy(P, hlow, lo, v);
}
DC_FN bool dcf_mirrored(const DCPlane &P, int mirror, int hlow, int rowleft, uint32_t &v) {
    if (hlow < 0 && (mirror & 1)) hlow = -hlow;
    if (hlow >= P.H && (mirror & 2)) hlow = P.H + P.H - hlow - 2;
    if (rowleft < 0 && (mirror & 4)) rowleft = -rowleft;
    if (rowleft >= P.W && (mirror & 8)) rowleft = P.W + P.W - rowleft - 2;
    if ((rowleft >= 0) && (rowleft < P.W) && (hlow >= 0) && (hlow < P.H)) return dcf_copy(P, hlow, rowleft, v);
    return dcf_border(P, v);
}

DC_FN bool dcf_nearest(const DCPlane &P, const DCCommon &C, int h, int row, uint32_t &v) {
    const int W = P.W, H = P.H;
    if (P.cls == 2) {
        float xsrc, ysrc;
        dc_chain(P, h, row, xsrc, ysrc);
        if (!dc_ok(xsrc) || !dc_ok(ysrc)) return dcf_border(P, v);
        int rowleft = (int)(xsrc + 0.5f);
        int hlow = (int)(ysrc + 0.5f);
        if ((rowleft >= 0) && (rowleft < W) && (hlow >= 0) && (hlow < H)) return dcf_copy(P, hlow, rowleft, v);
        return dcf_mirrored(P, C.mirror, hlow, rowleft, v);
    }
    int rowleft;
    float ysrc;
    if (P.cls == 0) {
        ysrc = P.dyc + h;
        if (!dc_ok(P.dxc)) return dcf_border(P, v);
        rowleft = (int)floorf(P.dxc + 0.5f) + row;
    } else {
        const float xsrc = P.dxc + P.dxx * row;
        ysrc = P.dyc + P.dyy * h;
        if (!dc_ok(xsrc)) return dcf_border(P, v);
        rowleft = (int)floorf(xsrc + 0.5f);
    }
    if (!dc_ok(ysrc)) return dcf_border(P, v);
    const int hlow = dc_mirror_row((int)floorf(ysrc + 0.5f), H, C.mirror);
    if ((hlow >= 0) && (hlow < H)) {
        if ((rowleft >= 0) && (rowleft < W)) return dcf_copy(P, hlow, rowleft, v);
        if (rowleft < 0 && (C.mirror & 4)) return dcf_left(P, hlow, rowleft, P.blur, v);
        if (rowleft >= W && (C.mirror & 8)) return dcf_right(P, hlow, rowleft, P.blur, 1, v);
    }
    return dcf_border(P, v);
}

// one formula for the three forms of bilinear; kx, ky in 32nds
DC_FN bool dcf_lerp(const DCPlane &P, int hlow, int rowleft, int kx, int ky, uint32_t &v) {
    const float fx = (float)kx, gx = (float)(32 - kx), fy = (float)ky, gy = (float)(32 - ky);
    const float top = gx * dcf_pf(P, hlow, rowleft) + fx * dcf_pf(P, hlow, rowleft + 1);
    const float bot = gx * dcf_pf(P, hlow + 1, rowleft) + fx * dcf_pf(P, hlow + 1, rowleft + 1);
    v = dcf_bits((gy * top + fy * bot) * (1.0f / 1024));
    return true;
}

DC_FN bool dcf_bilinear(const DCPlane &P, const DCCommon &C, int h, int row, uint32_t &v) {
    const int W = P.W, H = P.H;
    if (P.cls == 2) {
        float xsrc, ysrc;
        dc_chain(P, h, row, xsrc, ysrc);
        if (!dc_ok(xsrc) || !dc_ok(ysrc)) return dcf_border(P, v);
        int rowleft = (int)(xsrc);
        float sx = xsrc - rowleft;
        if (sx < 0) { sx += 1; rowleft -= 1; }
        int hlow = (int)(ysrc);
        float sy = ysrc - hlow;
        if (sy < 0) { sy += 1; hlow -= 1; }
        if ((rowleft >= 0) && (rowleft < W - 1) && (hlow >= 0) && (hlow < H - 1)) return dcf_lerp(P, hlow, rowleft, (int)(sx * 32), (int)(sy * 32), v);
        return dcf_mirrored(P, C.mirror, hlow, rowleft, v);
    }
    int rowleft, kx;
    float ysrc;
    if (P.cls == 0) {
        ysrc = P.dyc + h;
        if (!dc_ok(P.dxc)) return dcf_border(P, v);
        const int inttr0 = (int)floorf(P.dxc);
        kx = (int)floorf((P.dxc - inttr0) * 32);
        rowleft = inttr0 + row;
    } else {
        const float xsrc = P.dxc + P.dxx * row;
        ysrc = P.dyc + P.dyy * h;
        if (!dc_ok(xsrc)) return dcf_border(P, v);
        rowleft = (int)floorf(xsrc);
        kx = (int)floorf((xsrc - rowleft) * 32);
    }
    if (!dc_ok(ysrc)) return dcf_border(P, v);
    int hlow = (int)floorf(ysrc);
    const int ky = (int)floorf((ysrc - hlow) * 32);
    hlow = dc_mirror_row(hlow, H, C.mirror);
    if ((hlow >= 0) && (hlow < H - 1)) {
        if ((rowleft >= 0) && (rowleft < W - 1)) return dcf_lerp(P, hlow, rowleft, kx, ky, v);
        if (rowleft < 0 && (C.mirror & 4)) return dcf_left(P, hlow, rowleft, P.blur, v);
        if (rowleft >= W - 1 && (C.mirror & 8)) return dcf_right(P, hlow, rowleft, P.blur, 2, v);
    } else if (hlow == H - 1) {
        if ((rowleft >= 0) && (rowleft < W)) return dcf_copy(P, hlow, rowleft, v);
        if (P.cls == 0) {
            if (rowleft < 0 && (C.mirror & 4)) return dcf_left(P, hlow, rowleft, 0, v);
            if (rowleft >= W - 1 && (C.mirror & 8)) return dcf_right(P, hlow, rowleft, 0, 2, v);
        }
    }
    return dcf_border(P, v);
}

// one separable formula for the three forms of bicubic; ix, iy in 256ths.  The divisor is the weights' own sum, so a flat area stays flat.
DC_FN bool dcf_cubic(const DCPlane &P, int hlow, int rowleft, int ix, int iy, uint32_t &v) {
    const float cx0 = (float)dc_cub(ix, 0), cx1 = (float)dc_cub(ix, 1), cx2 = (float)dc_cub(ix, 2), cx3 = (float)dc_cub(ix, 3);
    float ts[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        ts[j] = cx0 * dcf_pf(P, hlow - 1 + j, rowleft - 1) + cx1 * dcf_pf(P, hlow - 1 + j, rowleft) + cx2 * dcf_pf(P, hlow - 1 + j, rowleft + 1) +
                cx3 * dcf_pf(P, hlow - 1 + j, rowleft + 2);
    const float pixel = (float)dc_cub(iy, 0) * ts[0] + (float)dc_cub(iy, 1) * ts[1] + (float)dc_cub(iy, 2) * ts[2] + (float)dc_cub(iy, 3) * ts[3];
    const int total = (dc_cub(ix, 0) + dc_cub(ix, 1) + dc_cub(ix, 2) + dc_cub(ix, 3)) * (dc_cub(iy, 0) + dc_cub(iy, 1) + dc_cub(iy, 2) + dc_cub(iy, 3));
    v = dcf_bits(pixel / (float)total);
    return true;
}
DC_FN bool dcf_edge(const DCPlane &P, int hlow, int rowleft, float sx, float sy, uint32_t &v) {
    v = dcf_bits((1.0f - sy) * ((1.0f - sx) * dcf_pf(P, hlow, rowleft) + sx * dcf_pf(P, hlow, rowleft + 1)) +
                 sy * ((1.0f - sx) * dcf_pf(P, hlow + 1, rowleft) + sx * dcf_pf(P, hlow + 1, rowleft + 1)));
    return true;
}

DC_FN bool dcf_bicubic(const DCPlane &P, const DCCommon &C, int h, int row, uint32_t &v) {
    const int W = P.W, H = P.H;
    if (P.cls == 2) {
        const float xsrc = P.dxc + P.dxx * row + P.dxy * h;
        const float ysrc = P.dyc + P.dyx * row + P.dyy * h;
        if (!dc_ok(xsrc) || !dc_ok(ysrc)) return dcf_border(P, v);
        int rowleft = (int)(xsrc);
        if (xsrc < rowleft) rowleft -= 1;
        int hlow = (int)(ysrc);
        if (ysrc < hlow) hlow -= 1;
        if ((rowleft >= 1) && (rowleft < W - 2) && (hlow >= 1) && (hlow < H - 2))
            return dcf_cubic(P, hlow, rowleft, (int)((xsrc - rowleft) * 256), (int)((ysrc - hlow) * 256), v);
        return dcf_mirrored(P, C.mirror, hlow, rowleft, v);
    }
    int rowleft, ix;
    float ysrc, sx, sy;
    if (P.cls == 0) {
        ysrc = P.dyc + h;
        if (!dc_ok(P.dxc) || !dc_ok(P.dyc)) return dcf_border(P, v);
        const int inttr0 = (int)floorf(P.dxc), inttr3 = (int)floorf(P.dyc);
        ix = (int)((P.dxc - inttr0) * 256);
        rowleft = inttr0 + row;
        sx = P.dxc - inttr0;
        sy = P.dyc - inttr3;
    } else {
        const float xsrc = P.dxc + P.dxx * row;
        ysrc = P.dyc + P.dyy * h;
        if (!dc_ok(xsrc)) return dcf_border(P, v);
        rowleft = (int)floorf(xsrc);
        ix = (int)((xsrc - rowleft) * 256);
        sx = xsrc - rowleft;
        sy = 0;
    }
    if (!dc_ok(ysrc)) return dcf_border(P, v);
    int hlow = (int)floorf(ysrc);
    const int iy = (int)((ysrc - hlow) * 256);
    if (P.cls == 1) sy = ysrc - hlow;
    hlow = dc_mirror_row(hlow, H, C.mirror);
    if ((hlow >= 1) && (hlow < H - 2)) {
        if ((rowleft >= 1) && (rowleft < W - 2)) return dcf_cubic(P, hlow, rowleft, ix, iy, v);
        if (rowleft < 0 && (C.mirror & 4)) return dcf_left(P, hlow, rowleft, P.blur, v);
        if (rowleft >= W && (C.mirror & 8)) return dcf_right(P, hlow, rowleft, P.blur, 1, v);
        if (rowleft == 0 || rowleft == W - 1 || rowleft == W - 2) return dcf_copy(P, hlow, rowleft, v);
    } else if (hlow == 0 || hlow == H - 2) {
        if ((rowleft >= 0) && (rowleft < W - 1)) return dcf_edge(P, hlow, rowleft, sx, sy, v);
        if (rowleft == W - 1) return dcf_copy(P, hlow, rowleft, v);
        if (rowleft < 0 && (C.mirror & 4)) return dcf_left(P, hlow, rowleft, 0, v);
        if (rowleft >= W && (C.mirror & 8)) return dcf_right(P, hlow, rowleft, 0, 1, v);
    } else if (hlow == H - 1) {
        if (rowleft >= 0 && rowleft < W) {
            if (P.cls != 1) return dcf_copy(P, hlow, rowleft, v);
            v = dcf_bits((dcf_pf(P, hlow, rowleft) + dcf_pf(P, hlow - 1, rowleft)) * 0.5f);
            return true;
        }
        if (rowleft < 0 && (C.mirror & 4)) return dcf_left(P, hlow, rowleft, 0, v);
        if (rowleft >= W && (C.mirror & 8)) return dcf_right(P, hlow, rowleft, 0, 1, v);
    }
    return dcf_border(P, v);
}

template <int SUB> DC_FN bool dcf_sample(const DCPlane &P, const DCCommon &C, int h, int row, uint32_t &v) {
    return SUB == 0 ? dcf_nearest(P, C, h, row, v) : SUB == 1 ? dcf_bilinear(P, C, h, row, v) : dcf_bicubic(P, C, h, row, v);
}

// DepanStabilise's selection, as ds_sample: the current frame, else next, else prev, by the painted flag.  Exactly the first pass painted
// carries a border value and the mirror bits, so the selection always ends painted.
template <int SUB> DC_FN bool dsf_sample(const DCPlane *S, const DCCommon &C, int h, int row, uint32_t &v) {
    const DCCommon none = { 0, C.pixel_max, C.nplanes };
    if (dcf_sample<SUB>(S[DS_CUR], S[DS_CUR].border >= 0 ? C : none, h, row, v)) return true;
    if (S[DS_NEXT].src && dcf_nearest(S[DS_NEXT], S[DS_NEXT].border >= 0 ? C : none, h, row, v)) return true;
    return S[DS_PREV].src && dcf_nearest(S[DS_PREV], C, h, row, v);
}

template <int SUB, int NSRC> DC_FN void dcf_store(const DCPlane *S, const DCCommon &C, int h, int row) {
    uint32_t v;
    if (NSRC == 1 ? dcf_sample<SUB>(S[0], C, h, row, v) : dsf_sample<SUB>(S, C, h, row, v))
        ((uint32_t *)(S[DS_CUR].dst + (long long)h * S[DS_CUR].dpitch))[row] = v;
}
