// mvx_depan_sample.h -- the warp of DepanCompensate and DepanStabilise for one output sample, and the host side of the records it reads:
// what depan_warp_kernel of mvx_depan_warp.hip runs per thread and what the two *_frames functions put into its table.
//   dc_nearest / dc_bilinear / dc_bicubic : compensate_plane_nearest / _bilinear / _bicubic, MVDepan.cpp:1626-2585, one DCPlane record.
//   ds_sample                             : DepanStabilise's selection among the up to three records of a plane (below).
//   dc_plane_transform, dc_fill, ds_borders (host) : a record from (plane, source, luma transform).
// It is a header without HIP so that tests/test_depan_ref.py and tests/test_depan_stab_ref.py can compile the same text for the host
// (tests/depan_warp_emu.cpp) and hold it to the restatements on a machine without a GPU.  Build with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>
#include <string.h>
#ifdef __HIPCC__
#define DC_FN __device__ __forceinline__
#else
#define DC_FN static inline
#endif
template <typename A> DC_FN A dc_min(A a, A b) { return a < b ? a : b; }
template <typename A> DC_FN A dc_max(A a, A b) { return a > b ? a : b; }

#define DC_SEG 64
#define DC_LIMIT 1073741824.0f

struct DCPlane {
    const unsigned char *src; unsigned char *dst;
    long long spitch, dpitch;             // bytes
    int W, H;
    float dxc, dxx, dxy, dyc, dyx, dyy;
    int border, blur, cls;                // cls: 0 translation, 1 zoom, 2 rotation
    float *chain;                         // cls 2 of nearest / bilinear: H * segs pairs
    int segs;
};
struct DCCommon { int mirror, pixel_max, nplanes; };

DC_FN bool dc_ok(float v) { return fabsf(v) < DC_LIMIT; } // false for NaN

// the walk of one row of a rotating plane, MVDepan.cpp:1804-1805,1840-1841 / :2136-2137,2186-2187: the pair before column 0, 64, 128, ...
DC_FN void dc_chain_row(const DCPlane &P, int h) {
    float xsrc = P.dxc + P.dxy * h, ysrc = P.dyc + P.dyy * h;
    float *c = P.chain + (size_t)h * P.segs * 2;
    const float dxx = P.dxx, dyx = P.dyx; // read once: the stores through c could alias P, and the walk would wait for two loads per column
    for (int row = 0; row < P.W; row++) {
        if ((row & (DC_SEG - 1)) == 0) { c[0] = xsrc; c[1] = ysrc; c += 2; }
        xsrc += dxx; ysrc += dyx;
    }
}

template <typename T> DC_FN int dc_px(const DCPlane &P, int y, int x) { return ((const T *)(P.src + (long long)y * P.spitch))[x]; }

// rowleft < 0 with MIRROR_LEFT in the forms that do not check the mirrored column: srcp[w0 - rowleft], or the mean of the blur run
// [-rowleft - blurlen + 1, -rowleft].  The run starts at 1 or later; it leaves the row when -rowleft >= row_size: border.
template <typename T> DC_FN int dc_left(const DCPlane &P, int hlow, int rowleft, int blurmax) {
    if (-rowleft >= P.W) return P.border;
    if (blurmax > 0) {
        const int blurlen = dc_min(blurmax, -rowleft);
        int smoothed = 0;
        for (int i = -rowleft - blurlen + 1; i <= -rowleft; i++) smoothed += dc_px<T>(P, hlow, i);
        return smoothed / blurlen;
    }
    return dc_px<T>(P, hlow, -rowleft);
}
// the right side: srcp[w0 + 2 * row_size - rowleft - 2], or the run of blurlen = dc_min(blurmax, rowleft - row_size + add) from there on, which
// ends at row_size - 1 or earlier; it starts before the row when rowleft > 2 * row_size - 2: border.
template <typename T> DC_FN int dc_right(const DCPlane &P, int hlow, int rowleft, int blurmax, int add) {
    const int lo = P.W + P.W - rowleft - 2;
    if (lo < 0) return P.border;
    if (blurmax > 0) {
        const int blurlen = dc_min(blurmax, rowleft - P.W + add);
        int smoothed = 0;
        for (int i = lo; i < lo + blurlen; i++) smoothed += dc_px<T>(P, hlow, i);
        return smoothed / blurlen;
    }
    return dc_px<T>(P, hlow, lo);
}
// the rotation forms' mirror: every index is checked after it (:1825-1838, :2171-2184, :2565-2578)
template <typename T> DC_FN int dc_mirrored(const DCPlane &P, int mirror, int hlow, int rowleft) {
    if (hlow < 0 && (mirror & 1)) hlow = -hlow;
    if (hlow >= P.H && (mirror & 2)) hlow = P.H + P.H - hlow - 2;
    if (rowleft < 0 && (mirror & 4)) rowleft = -rowleft;
    if (rowleft >= P.W && (mirror & 8)) rowleft = P.W + P.W - rowleft - 2;
    if ((rowleft >= 0) && (rowleft < P.W) && (hlow >= 0) && (hlow < P.H)) return dc_px<T>(P, hlow, rowleft);
    return P.border;
}
DC_FN int dc_mirror_row(int hlow, int H, int mirror) {
    if (hlow < 0 && (mirror & 1)) hlow = -hlow;
    if (hlow >= H && (mirror & 2)) hlow = H + H - hlow - 2;
    return hlow;
}
// the checkpointed walk of the rotation forms of nearest and bilinear
DC_FN void dc_chain(const DCPlane &P, int h, int row, float &xsrc, float &ysrc) {
    const float *c = P.chain + ((size_t)h * P.segs + (row / DC_SEG)) * 2;
    xsrc = c[0]; ysrc = c[1];
    for (int k = row & (DC_SEG - 1); k > 0; k--) { xsrc += P.dxx; ysrc += P.dyx; }
}

// compensate_plane_nearest, MVDepan.cpp:1626-1847
template <typename T> DC_FN int dc_nearest(const DCPlane &P, const DCCommon &C, int h, int row) {
    const int W = P.W, H = P.H;
    if (P.cls == 2) {
        float xsrc, ysrc;
        dc_chain(P, h, row, xsrc, ysrc);
        if (!dc_ok(xsrc) || !dc_ok(ysrc)) return P.border;
        int rowleft = (int)(xsrc + 0.5f);
        int hlow = (int)(ysrc + 0.5f);
        if ((rowleft >= 0) && (rowleft < W) && (hlow >= 0) && (hlow < H)) return dc_px<T>(P, hlow, rowleft);
        return dc_mirrored<T>(P, C.mirror, hlow, rowleft);
    }
    int rowleft;
    float ysrc;
    if (P.cls == 0) {
        ysrc = P.dyc + h;
        if (!dc_ok(P.dxc)) return P.border;
        rowleft = (int)floorf(P.dxc + 0.5f) + row;
    } else {
        const float xsrc = P.dxc + P.dxx * row;
        ysrc = P.dyc + P.dyy * h;
        if (!dc_ok(xsrc)) return P.border;
        rowleft = (int)floorf(xsrc + 0.5f);
    }
    if (!dc_ok(ysrc)) return P.border;
    const int hlow = dc_mirror_row((int)floorf(ysrc + 0.5f), H, C.mirror);
    if ((hlow >= 0) && (hlow < H)) {
        if ((rowleft >= 0) && (rowleft < W)) return dc_px<T>(P, hlow, rowleft);
        if (rowleft < 0 && (C.mirror & 4)) return dc_left<T>(P, hlow, rowleft, P.blur);
        if (rowleft >= W && (C.mirror & 8)) return dc_right<T>(P, hlow, rowleft, P.blur, 1);
    }
    return P.border;
}

// compensate_plane_bilinear, MVDepan.cpp:1855-2193.  intcoef[2 * k] = 32 - k, intcoef[2 * k + 1] = k.
template <typename T> DC_FN int dc_bilinear(const DCPlane &P, const DCCommon &C, int h, int row) {
    const int W = P.W, H = P.H;
    if (P.cls == 2) {
        float xsrc, ysrc;
        dc_chain(P, h, row, xsrc, ysrc);
        if (!dc_ok(xsrc) || !dc_ok(ysrc)) return P.border;
        int rowleft = (int)(xsrc);
        float sx = xsrc - rowleft;
        if (sx < 0) { sx += 1; rowleft -= 1; }
        int hlow = (int)(ysrc);
        float sy = ysrc - hlow;
        if (sy < 0) { sy += 1; hlow -= 1; }
        if ((rowleft >= 0) && (rowleft < W - 1) && (hlow >= 0) && (hlow < H - 1)) {
            const int kx = (int)(sx * 32), ky = (int)(sy * 32);
            return ((((32 - kx) * dc_px<T>(P, hlow, rowleft) + kx * dc_px<T>(P, hlow, rowleft + 1)) * (32 - ky) +
                     ((32 - kx) * dc_px<T>(P, hlow + 1, rowleft) + kx * dc_px<T>(P, hlow + 1, rowleft + 1)) * ky) >> 10);
        }
        return dc_mirrored<T>(P, C.mirror, hlow, rowleft);
    }
    int rowleft, kx;
    float ysrc;
    if (P.cls == 0) {
        ysrc = P.dyc + h;
        if (!dc_ok(P.dxc)) return P.border;
        const int inttr0 = (int)floorf(P.dxc);
        kx = (int)floorf((P.dxc - inttr0) * 32);
        rowleft = inttr0 + row;
    } else {
        const float xsrc = P.dxc + P.dxx * row;
        ysrc = P.dyc + P.dyy * h;
        if (!dc_ok(xsrc)) return P.border;
        rowleft = (int)floorf(xsrc);
        kx = (int)floorf((xsrc - rowleft) * 32);
    }
    if (!dc_ok(ysrc)) return P.border;
    int hlow = (int)floorf(ysrc);
    const int ky = (int)floorf((ysrc - hlow) * 32);
    hlow = dc_mirror_row(hlow, H, C.mirror);
    if ((hlow >= 0) && (hlow < H - 1)) {
        if ((rowleft >= 0) && (rowleft < W - 1))
            return ((32 - ky) * (32 - kx) * dc_px<T>(P, hlow, rowleft) + (32 - ky) * kx * dc_px<T>(P, hlow, rowleft + 1) +
                    ky * (32 - kx) * dc_px<T>(P, hlow + 1, rowleft) + ky * kx * dc_px<T>(P, hlow + 1, rowleft + 1)) >> 10;
        if (rowleft < 0 && (C.mirror & 4)) return dc_left<T>(P, hlow, rowleft, P.blur);
        if (rowleft >= W - 1 && (C.mirror & 8)) return dc_right<T>(P, hlow, rowleft, P.blur, 2);
    } else if (hlow == H - 1) {
        if ((rowleft >= 0) && (rowleft < W)) return dc_px<T>(P, hlow, rowleft);
        if (P.cls == 0) { // :2011-2014; the zoom form has no mirror on this row (:2116-2120)
            if (rowleft < 0 && (C.mirror & 4)) return dc_left<T>(P, hlow, rowleft, 0);
            if (rowleft >= W - 1 && (C.mirror & 8)) return dc_right<T>(P, hlow, rowleft, 0, 2);
        }
    }
    return P.border;
}

// bicubic's table, MVDepan.cpp:2255-2260: entry k (0..3) of step i (0..256)
DC_FN int dc_cub(int i, int k) {
    if (k == 0) return -((i * (256 - i) * (256 - i))) / 8192;
    if (k == 1) return (256 * 256 * 256 - 2 * 256 * i * i + i * i * i) / 8192;
    if (k == 2) return (i * (256 * 256 + 256 * i - i * i)) / 8192;
    return -(i * i * (256 - i)) / 8192;
}
// :2426-2438, :2549-2563: the separable form of the zoom and rotation forms, accumulated in 64 bits
template <typename T> DC_FN int dc_cubic_sep(const DCPlane &P, int pixel_max, int hlow, int rowleft, int ix, int iy) {
    long long ts[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        ts[j] = (dc_cub(ix, 0) * dc_px<T>(P, hlow - 1 + j, rowleft - 1) + dc_cub(ix, 1) * dc_px<T>(P, hlow - 1 + j, rowleft) +
                 dc_cub(ix, 2) * dc_px<T>(P, hlow - 1 + j, rowleft + 1) + dc_cub(ix, 3) * dc_px<T>(P, hlow - 1 + j, rowleft + 2));
    const long long pixel = (dc_cub(iy, 0) * ts[0] + dc_cub(iy, 1) * ts[1] + dc_cub(iy, 2) * ts[2] + dc_cub(iy, 3) * ts[3]) >> 22;
    return (int)dc_max(dc_min(pixel, (long long)pixel_max), 0ll);
}
// :2347-2348, :2472-2473: the near-edge rows, in double
template <typename T> DC_FN int dc_edge_double(const DCPlane &P, int hlow, int rowleft, float sx, float sy) {
    return (int)((1.0 - sy) * ((1.0 - sx) * dc_px<T>(P, hlow, rowleft) + sx * dc_px<T>(P, hlow, rowleft + 1)) +
                 sy * ((1.0 - sx) * dc_px<T>(P, hlow + 1, rowleft) + sx * dc_px<T>(P, hlow + 1, rowleft + 1)));
}

// compensate_plane_bicubic, MVDepan.cpp:2202-2585
template <typename T> DC_FN int dc_bicubic(const DCPlane &P, const DCCommon &C, int h, int row) {
    const int W = P.W, H = P.H;
    if (P.cls == 2) {
        const float xsrc = P.dxc + P.dxx * row + P.dxy * h;
        const float ysrc = P.dyc + P.dyx * row + P.dyy * h;
        if (!dc_ok(xsrc) || !dc_ok(ysrc)) return P.border;
        int rowleft = (int)(xsrc);
        if (xsrc < rowleft) rowleft -= 1;
        int hlow = (int)(ysrc);
        if (ysrc < hlow) hlow -= 1;
        if ((rowleft >= 1) && (rowleft < W - 2) && (hlow >= 1) && (hlow < H - 2))
            return dc_cubic_sep<T>(P, C.pixel_max, hlow, rowleft, (int)((xsrc - rowleft) * 256), (int)((ysrc - hlow) * 256));
        return dc_mirrored<T>(P, C.mirror, hlow, rowleft);
    }
    int rowleft, ix;
    float ysrc, sx, sy;
    if (P.cls == 0) {
        ysrc = P.dyc + h;
        if (!dc_ok(P.dxc) || !dc_ok(P.dyc)) return P.border;
        const int inttr0 = (int)floorf(P.dxc), inttr3 = (int)floorf(P.dyc);
        ix = (int)((P.dxc - inttr0) * 256);
        rowleft = inttr0 + row;
        sx = P.dxc - inttr0;
        sy = P.dyc - inttr3;
    } else {
        const float xsrc = P.dxc + P.dxx * row;
        ysrc = P.dyc + P.dyy * h;
        if (!dc_ok(xsrc)) return P.border;
        rowleft = (int)floorf(xsrc);
        ix = (int)((xsrc - rowleft) * 256);
        sx = xsrc - rowleft;
        sy = 0;
    }
    if (!dc_ok(ysrc)) return P.border;
    int hlow = (int)floorf(ysrc);
    const int iy = (int)((ysrc - hlow) * 256);
    if (P.cls == 1) sy = ysrc - hlow;
    hlow = dc_mirror_row(hlow, H, C.mirror);
    if ((hlow >= 1) && (hlow < H - 2)) {
        if ((rowleft >= 1) && (rowleft < W - 2)) {
            if (P.cls == 1) return dc_cubic_sep<T>(P, C.pixel_max, hlow, rowleft, ix, iy);
            int pixel = 1024; // :2281,2305-2311: sixteen coefficients, each the product / 2048 truncated towards zero, accumulated in int
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int i = 0; i < 4; i++) pixel += ((dc_cub(iy, j) * dc_cub(ix, i)) / 2048) * dc_px<T>(P, hlow - 1 + j, rowleft - 1 + i);
            pixel >>= 11;
            return dc_max(dc_min(pixel, C.pixel_max), 0);
        }
        if (rowleft < 0 && (C.mirror & 4)) return dc_left<T>(P, hlow, rowleft, P.blur);
        if (rowleft >= W && (C.mirror & 8)) return dc_right<T>(P, hlow, rowleft, P.blur, 1);
        if (rowleft == 0 || rowleft == W - 1 || rowleft == W - 2) return dc_px<T>(P, hlow, rowleft);
    } else if (hlow == 0 || hlow == H - 2) {
        if ((rowleft >= 0) && (rowleft < W - 1)) {
            const int pixel = dc_edge_double<T>(P, hlow, rowleft, sx, sy);
            return P.cls == 1 ? dc_max(dc_min(pixel, C.pixel_max), 0) : pixel;
        }
        if (rowleft == W - 1) return dc_px<T>(P, hlow, rowleft);
        if (rowleft < 0 && (C.mirror & 4)) return dc_left<T>(P, hlow, rowleft, 0);
        if (rowleft >= W && (C.mirror & 8)) return dc_right<T>(P, hlow, rowleft, 0, 1);
    } else if (hlow == H - 1) {
        if (rowleft >= 0 && rowleft < W) return P.cls == 1 ? (dc_px<T>(P, hlow, rowleft) + dc_px<T>(P, hlow - 1, rowleft)) / 2 : dc_px<T>(P, hlow, rowleft);
        if (rowleft < 0 && (C.mirror & 4)) return dc_left<T>(P, hlow, rowleft, 0);
        if (rowleft >= W && (C.mirror & 8)) return dc_right<T>(P, hlow, rowleft, 0, 1);
    }
    return P.border;
}

template <typename T, int SUB> DC_FN int dc_sample(const DCPlane &P, const DCCommon &C, int h, int row) {
    return SUB == 0 ? dc_nearest<T>(P, C, h, row) : SUB == 1 ? dc_bilinear<T>(P, C, h, row) : dc_bicubic<T>(P, C, h, row);
}

// ------------------------------------------------------------------------------------------------ DepanStabilise's selection
// The reference paints one destination up to three times (MVDepan.cpp:3679-3693): fillBorderPrev (nearest, the filter's mirror, the border
// value), fillBorderNext (nearest; border -1 and no mirror once prev has painted), compensateFrame (the subpixel interpolator; border -1 and
// no mirror once anything has painted).  A pass with border -1 leaves a sample alone where its position is outside its source, and every
// pass writes a pure function of its own source, so the last pass that holds a sample decides it: the current frame, else next, else prev.
// A plane's three sources lie side by side, S[DS_CUR], S[DS_NEXT], S[DS_PREV]; an unused one has src == nullptr.  Exactly the first pass
// painted carries a border value >= 0 and the mirror bits, so the selection always ends on a value >= 0.
enum { DS_CUR = 0, DS_NEXT = 1, DS_PREV = 2, DS_SOURCES = 3 };

template <typename T, int SUB> DC_FN int ds_sample(const DCPlane *S, const DCCommon &C, int h, int row) {
    const DCCommon none = { 0, C.pixel_max, C.nplanes };
    int v = dc_sample<T, SUB>(S[DS_CUR], S[DS_CUR].border >= 0 ? C : none, h, row);
    if (v < 0 && S[DS_NEXT].src) v = dc_nearest<T>(S[DS_NEXT], S[DS_NEXT].border >= 0 ? C : none, h, row);
    if (v < 0 && S[DS_PREV].src) v = dc_nearest<T>(S[DS_PREV], C, h, row);
    return v;
}

// one output sample of a plane with NSRC records: 1 DepanCompensate, DS_SOURCES DepanStabilise
template <typename T, int SUB, int NSRC> DC_FN void dc_store(const DCPlane *S, const DCCommon &C, int h, int row) {
    const int v = NSRC == 1 ? dc_sample<T, SUB>(S[0], C, h, row) : ds_sample<T, SUB>(S, C, h, row);
    ((T *)(S[DS_CUR].dst + (long long)h * S[DS_CUR].dpitch))[row] = (T)v;
}

// ------------------------------------------------------------------------------------------------ the host side of a record
// what a filter's records share: the clip's geometry per plane, the pitches, and the arguments that both filters take
struct DCClip {
    int bits, np, ssw, ssh, subpixel, mirror, pixel_max;
    int W[3], H[3], border[3], blur[3];
    long long spitch[3], dpitch[3];
};

// plane p's transform from the pass's luma transform, MVDepan.cpp:2687-2700 / :3366-3379, and its form, the comparisons of :1666,1733 (the
// same in all three interpolators); tr: dxc dxx dxy dyc dyx dyy
static inline void dc_plane_transform(int ssw, int ssh, int p, const float *tr, DCPlane *P) {
    float dxc = tr[0], dxx = tr[1], dxy = tr[2], dyc = tr[3], dyx = tr[4], dyy = tr[5];
    if (p && ssw == 1 && ssh == 1) { dxc /= 2; dyc /= 2; }
    else if (p && ssw == 1 && ssh == 0) { dxc /= 2; dxy /= 2; dyx *= 2; }
    P->dxc = dxc; P->dxx = dxx; P->dxy = dxy; P->dyc = dyc; P->dyx = dyx; P->dyy = dyy;
    P->cls = (dxy == 0.0f && dyx == 0.0f && dxx == 1.0f && dyy == 1.0f) ? 0 : (dxy == 0.0f && dyx == 0.0f) ? 1 : 2;
}

// the record of plane p read from src by the luma transform tr, with the border value of a first pass.  fill: a fill source of
// DepanStabilise, nearest whatever subpixel is.  Returns the number of floats of the chain the record needs (the rotation form of nearest
// and bilinear) and leaves P->chain to the caller.
static inline size_t dc_fill(const DCClip &G, int p, const void *src, void *dst, const float *tr, bool fill, DCPlane *P) {
    memset(P, 0, sizeof(*P));
    P->src = (const unsigned char *)src; P->dst = (unsigned char *)dst;
    P->spitch = G.spitch[p]; P->dpitch = G.dpitch[p];
    P->W = G.W[p]; P->H = G.H[p];
    P->border = G.border[p]; P->blur = G.blur[p];
    dc_plane_transform(G.ssw, G.ssh, p, tr, P);
    P->segs = (P->W + DC_SEG - 1) / DC_SEG;
    return P->cls == 2 && (fill || G.subpixel < 2) ? (size_t)P->H * P->segs * 2 : 0;
}

// border values of the passes of one plane: `border` for the first pass painted (prev, else next, else the current frame), -1 for the others
static inline void ds_borders(DCPlane *S, int border) {
    S[DS_PREV].border = border;
    S[DS_NEXT].border = S[DS_PREV].src ? -1 : border;
    S[DS_CUR].border = S[DS_PREV].src || S[DS_NEXT].src ? -1 : border;
}
