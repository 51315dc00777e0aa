// mvx_depan_fft_core.h -- the text of DepanEstimate's five passes (mvx_depan_fft.hip), written so that a host compiler runs the same
// arithmetic in the same order: a pass is a sequence of phases, DE_FOR(t, total) spreads a phase's `total` independent items over the
// workgroup's threads (on the host: a plain loop), DE_SYNC() separates phases.  tests/depan_fft_emu.cpp includes this header and runs
// the passes on the CPU; with -ffp-contract=off on both sides every float of it equals the kernel's.
//
// One LDS routine serves all four transforms: de_fft does C independent radix-2 decimation-in-time FFTs of length n at once, element j of
// transform c at [j * C + c], real and imaginary parts in separate float arrays.  A butterfly item t takes c = t % C, so the lanes of a wave walk
// the transforms first: with C >= 32 every stage is free of bank conflicts whatever its stride; with fewer (n >= 512) the first
// log2(32 / C) stages are 2-way conflicted, the rest free.  C = clamp(8192 / n, 1, 32): at most 8192 complex values = 64 KiB per workgroup.
//   rows, forward   : two window rows ride one complex transform (row a real, row b imaginary) and are separated afterwards
//   columns, forward: C adjacent columns of the half spectrum per workgroup, in place
//   columns, inverse: the conjugate product of two spectra is formed on load; only the rows the peak search can read are stored
//   rows, inverse   : two kept rows ride one complex transform (Z = A + iB of their Hermitian extensions)
//   peak            : one workgroup per window: the maximum by 256 strided partial results and a fixed tree, the sum by the reference's serial chain
//   show            : over a surface with every row kept (nrows = winy, jshift = 0): minimum and maximum by strided partial results and fixed trees
//                     (either is the same in any order), then the surface painted into the window of a luma plane (showcorrelation, MVDepan.cpp:895-953)
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DE_DEV __device__ static inline
#define DE_FOR(t, total) for (int t = (int)threadIdx.x; t < (total); t += (int)blockDim.x)
#define DE_SYNC() __syncthreads()
#else
#define DE_DEV static inline
#define DE_FOR(t, total) for (int t = 0; t < (total); t++)
#define DE_SYNC() ((void)0)
#endif

#define DE_THREADS 256
#define DE_LDS_COMPLEX 8192 // complex values a workgroup holds: 64 KiB
#define DE_MAX_BATCH 32     // transforms per workgroup: one per LDS bank of a 4-byte access

struct alignas(8) DEComplex { float x, y; };

// what the scan of one correlation surface leaves for the host tail (get_motion_vector from `trust` on, MVDepan.cpp:769-882)
struct DEScan {
    float max, sum;     // the first maximum in scan order and the sum over the four corners, both unnormalised
    int32_t imax, jmax;
    float xp, xm, yp, ym; // the surface at (imax + 1, jmax), (imax - 1, jmax), (imax, jmax + 1), (imax, jmax - 1), wrapped
};

struct DEParams {
    int winx, winy, nx;       // nx = winx / 2 + 1 complex values per spectrum row
    int lgx, lgy;             // log2 of winx, winy
    int cx, lgcx, cy, lgcy;   // transforms per workgroup of the row passes (length winx) and of the column passes (length winy)
    int nwin, wleft[2], wtop;
    int dxmax, dymax;
    int nrows, jshift;        // rows of the correlation surface that are kept: 0 .. dymax + 1 and winy - dymax - 1 .. winy - 1
    int bits16;
    long long pitch;          // bytes
};

// tw[k] = exp(-2 pi i k / n), k < n / 2: in double, rounded to float once; k = n / 4 is exactly -i
static inline void de_twiddles(DEComplex *tw, int n) {
    for (int k = 0; k < n / 2; k++) {
        const double a = -2.0 * 3.14159265358979323846264338327950288 * (double)k / (double)n;
        tw[k].x = (float)cos(a); tw[k].y = (float)sin(a);
    }
    if (n >= 4) { tw[n / 4].x = 0.0f; tw[n / 4].y = -1.0f; }
}

static inline int de_batch(int n) { const int c = DE_LDS_COMPLEX / n; return c < 1 ? 1 : c > DE_MAX_BATCH ? DE_MAX_BATCH : c; }

// surface row j -> its row among the kept ones (j must be a kept row)
DE_DEV int de_kept(const DEParams &P, int j) { return j <= P.dymax + 1 ? j : j - P.jshift; }
DE_DEV int de_row_of_kept(const DEParams &P, int r) { return r <= P.dymax + 1 ? r : r + P.jshift; }

DE_DEV unsigned de_bitrev(unsigned v, int bits) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - bits);
}

// C = 1 << lgc transforms of length n = 1 << lg over bit-reversed input; tw[k] = exp(-2 pi i k / n), k < n / 2.  Unnormalised both ways.
DE_DEV void de_fft(float *re, float *im, const DEComplex *tw, int lg, int lgc, int inverse) {
    const int total = (1 << (lg - 1)) << lgc, cmask = (1 << lgc) - 1;
    for (int s = 0; s < lg; s++) {
        const int h = 1 << s;
        DE_FOR(t, total) {
            const int c = t & cmask, u = t >> lgc, k = u & (h - 1);
            const int a = ((((u >> s) << (s + 1)) + k) << lgc) + c, b = a + (h << lgc);
            const DEComplex w = tw[k << (lg - 1 - s)];
            const float wr = w.x, wi = inverse ? -w.y : w.y;
            const float xr = re[b], xi = im[b];
            const float tr = xr * wr - xi * wi, ti = xr * wi + xi * wr;
            const float ur = re[a], ui = im[a];
            re[a] = ur + tr; im[a] = ui + ti;
            re[b] = ur - tr; im[b] = ui - ti;
        }
        DE_SYNC();
    }
}

DE_DEV float de_sample(const DEParams &P, const unsigned char *plane, int win, int row, int x) {
    const unsigned char *p = plane + (long long)(P.wtop + row) * P.pitch;
    const int i = P.wleft[win] + x;
    return P.bits16 ? (float)((const unsigned short *)p)[i] : (float)p[i];
}

// rows 2p and 2p + 1 of the window, p = group * cx ..: spec[row][k], k <= winx / 2, of each
DE_DEV void de_rows_forward(const DEParams &P, const unsigned char *plane, int win, int group, DEComplex *spec, const DEComplex *twx, float *re, float *im) {
    const int n = P.winx, C = P.cx, pairs = P.winy >> 1, p0 = group * C;
    DE_FOR(t, n << P.lgcx) {
        const int x = t & (n - 1), c = t >> P.lgx, p = p0 + c;
        const int d = ((int)de_bitrev((unsigned)x, P.lgx) << P.lgcx) + c;
        re[d] = p < pairs ? de_sample(P, plane, win, 2 * p, x) : 0.0f;
        im[d] = p < pairs ? de_sample(P, plane, win, 2 * p + 1, x) : 0.0f;
    }
    DE_SYNC();
    de_fft(re, im, twx, P.lgx, P.lgcx, 0);
    DE_FOR(t, P.nx * C) {
        const int c = t / P.nx, k = t - c * P.nx, p = p0 + c;
        if (p < pairs) {
            const int a = (k << P.lgcx) + c, b = (((n - k) & (n - 1)) << P.lgcx) + c;
            const float zr = re[a], zi = im[a], yr = re[b], yi = im[b];
            // A[k] = (Z[k] + conj(Z[n - k])) / 2, B[k] = (Z[k] - conj(Z[n - k])) / 2i
            spec[(long long)(2 * p) * P.nx + k] = DEComplex{0.5f * (zr + yr), 0.5f * (zi - yi)};
            spec[(long long)(2 * p + 1) * P.nx + k] = DEComplex{0.5f * (zi + yi), 0.5f * (yr - zr)};
        }
    }
}

// columns group * cy .. of the half spectrum, in place
DE_DEV void de_cols_forward(const DEParams &P, int group, DEComplex *spec, const DEComplex *twy, float *re, float *im) {
    const int n = P.winy, C = P.cy, k0 = group * C;
    DE_FOR(t, n << P.lgcy) {
        const int c = t & (C - 1), j = t >> P.lgcy, k = k0 + c;
        const int d = ((int)de_bitrev((unsigned)j, P.lgy) << P.lgcy) + c;
        const DEComplex v = k < P.nx ? spec[(long long)j * P.nx + k] : DEComplex{0.0f, 0.0f};
        re[d] = v.x; im[d] = v.y;
    }
    DE_SYNC();
    de_fft(re, im, twy, P.lgy, P.lgcy, 0);
    DE_FOR(t, n << P.lgcy) {
        const int c = t & (C - 1), j = t >> P.lgcy, k = k0 + c;
        if (k < P.nx) spec[(long long)j * P.nx + k] = DEComplex{re[t], im[t]};
    }
}

// the product of mult_conj_data2d (MVDepan.cpp:689-691: fftnext = cur, fftsrc = prev) on load, the inverse transform of the columns, and the kept
// rows of the result to half[kept row][k]
DE_DEV void de_cols_correlate(const DEParams &P, int group, const DEComplex *cur, const DEComplex *prev, DEComplex *half, const DEComplex *twy, float *re, float *im) {
    const int n = P.winy, C = P.cy, k0 = group * C;
    DE_FOR(t, n << P.lgcy) {
        const int c = t & (C - 1), j = t >> P.lgcy, k = k0 + c;
        const int d = ((int)de_bitrev((unsigned)j, P.lgy) << P.lgcy) + c;
        float mr = 0.0f, mi = 0.0f;
        if (k < P.nx) {
            const DEComplex a = cur[(long long)j * P.nx + k], b = prev[(long long)j * P.nx + k];
            mr = a.x * b.x + a.y * b.y;
            mi = a.x * b.y - a.y * b.x;
        }
        re[d] = mr; im[d] = mi;
    }
    DE_SYNC();
    de_fft(re, im, twy, P.lgy, P.lgcy, 1);
    DE_FOR(t, P.nrows << P.lgcy) {
        const int c = t & (C - 1), r = t >> P.lgcy, k = k0 + c;
        const int a = (de_row_of_kept(P, r) << P.lgcy) + c;
        if (k < P.nx) half[(long long)r * P.nx + k] = DEComplex{re[a], im[a]};
    }
}

// kept rows 2q and 2q + 1, q = group * cx ..: the real inverse transform of each (the imaginary parts of bins 0 and winx / 2 are not read,
// as in a c2r transform) to corr[kept row][x]
DE_DEV void de_rows_inverse(const DEParams &P, int group, const DEComplex *half, float *corr, const DEComplex *twx, float *re, float *im) {
    const int n = P.winx, C = P.cx, q0 = group * C;
    DE_FOR(t, n << P.lgcx) {
        const int x = t & (n - 1), c = t >> P.lgx, ra = 2 * (q0 + c), rb = ra + 1;
        const int k = x <= (n >> 1) ? x : n - x;
        const bool edge = k == 0 || k == (n >> 1);
        DEComplex A = {0.0f, 0.0f}, B = {0.0f, 0.0f};
        if (ra < P.nrows) A = half[(long long)ra * P.nx + k];
        if (rb < P.nrows) B = half[(long long)rb * P.nx + k];
        if (edge) { A.y = 0.0f; B.y = 0.0f; }
        if (x > (n >> 1)) { A.y = -A.y; B.y = -B.y; }
        const int d = ((int)de_bitrev((unsigned)x, P.lgx) << P.lgcx) + c;
        re[d] = A.x - B.y; im[d] = A.y + B.x;
    }
    DE_SYNC();
    de_fft(re, im, twx, P.lgx, P.lgcx, 1);
    DE_FOR(t, n << P.lgcx) {
        const int x = t & (n - 1), c = t >> P.lgx, ra = 2 * (q0 + c), rb = ra + 1;
        const int a = (x << P.lgcx) + c;
        if (ra < P.nrows) corr[(long long)ra * n + x] = re[a];
        if (rb < P.nrows) corr[(long long)rb * n + x] = im[a];
    }
}

// the value at place q of the scan of get_motion_vector, MVDepan.cpp:717-767: rows 0 .. dymax then winy - dymax .. winy - 1, in each columns 0 .. dxmax
// then winx - dxmax .. winx - 1
DE_DEV void de_scan_place(const DEParams &P, int q, int *i, int *j) {
    const int wrow = 2 * P.dxmax + 1, r = q / wrow, p = q - r * wrow;
    *i = p <= P.dxmax ? p : P.winx - wrow + p;
    *j = r <= P.dymax ? r : P.winy - (2 * P.dymax + 1) + r;
}
DE_DEV float de_scan_value(const DEParams &P, const float *corr, int q) {
    int i, j;
    de_scan_place(P, q, &i, &j);
    return corr[(long long)de_kept(P, j) * P.winx + i];
}

// The scan over q = 0 .. count - 1.  The first maximum is the largest value at the lowest q: 256 strided partial results, merged by halving.
// The sum for the mean is the reference's own chain, correlmean += cur in scan order in float (:724, :734, :748, :758): another order gives another
// float, and on a large search area the difference in trust exceeds what two FFTs differ by.  So one thread adds, in order, out of LDS, while the
// other three waves stage the next DE_CHUNK values (the rest of the adding thread's own wave does not: its lanes would run after the chain, in
// front of the barrier).  The measured cost is in DESIGN.md 4.11.
#define DE_CHUNK 4096
DE_DEV void de_peak(const DEParams &P, const float *corr, DEScan *out, float *stage, float *lmax, int *lidx) {
    const int count = (2 * P.dxmax + 1) * (2 * P.dymax + 1);
    DE_FOR(l, DE_THREADS) {
        float best = 0.0f;
        int bi = -1;
        for (int q = l; q < count; q += DE_THREADS) {
            const float v = de_scan_value(P, corr, q);
            if (bi < 0 || v > best) { best = v; bi = q; }
        }
        lmax[l] = best; lidx[l] = bi;
    }
    DE_FOR(t, DE_CHUNK) if (t < count) stage[t] = de_scan_value(P, corr, t);
    DE_SYNC();
    for (int w = DE_THREADS / 2; w > 0; w >>= 1) {
        DE_FOR(l, w) {
            const int o = l + w;
            if (lidx[o] >= 0 && (lidx[l] < 0 || lmax[o] > lmax[l] || (lmax[o] == lmax[l] && lidx[o] < lidx[l]))) { lmax[l] = lmax[o]; lidx[l] = lidx[o]; }
        }
        DE_SYNC();
    }
    float sum = 0.0f; // thread 0's
    for (int q0 = 0, k = 0; q0 < count; q0 += DE_CHUNK, k++) {
        const float *cur = stage + (k & 1) * DE_CHUNK;
        float *next = stage + ((k + 1) & 1) * DE_CHUNK;
        const int n = count - q0 < DE_CHUNK ? count - q0 : DE_CHUNK, q1 = q0 + DE_CHUNK;
        const int n1 = q1 >= count ? 0 : count - q1 < DE_CHUNK ? count - q1 : DE_CHUNK;
        DE_FOR(t, DE_THREADS) {
            if (t == 0)
                for (int i = 0; i < n; i++) sum += cur[i];
            else if (t >= 64)
                for (int i = t - 64; i < n1; i += DE_THREADS - 64) next[i] = de_scan_value(P, corr, q1 + i);
        }
        DE_SYNC();
    }
    DE_FOR(l, 1) {
        int i, j;
        de_scan_place(P, lidx[0] < 0 ? 0 : lidx[0], &i, &j); // only a surface of NaNs leaves no maximum: the reference keeps (0, 0) then
        const int ip = i + 1 < P.winx ? i + 1 : 0, im1 = i >= 1 ? i - 1 : P.winx - 1;
        const int jp = j + 1 < P.winy ? j + 1 : 0, jm = j >= 1 ? j - 1 : P.winy - 1;
        const long long row = (long long)de_kept(P, j) * P.winx;
        DEScan S;
        S.max = corr[row + i]; S.sum = sum; S.imax = i; S.jmax = j;
        S.xp = corr[row + ip]; S.xm = corr[row + im1];
        S.yp = corr[(long long)de_kept(P, jp) * P.winx + i]; S.ym = corr[(long long)de_kept(P, jm) * P.winx + i];
        *out = S;
    }
}

// ---- show, MVDepan.cpp:895-953, on a surface of winy full rows.  Minimum and maximum: `groups` workgroups per window, each over the values
// group * DE_THREADS + l, stepping groups * DE_THREADS, merged by halving; partial[2 * group] and [2 * group + 1] hold its minimum and maximum.
#define DE_SHOW_GROUPS DE_THREADS // at most: the paint merges the partial results with one tree of DE_THREADS places
static inline int de_show_groups(int total) { const int g = (total + 4095) / 4096; return g < 1 ? 1 : g > DE_SHOW_GROUPS ? DE_SHOW_GROUPS : g; }

DE_DEV void de_minmax_tree(float *lmin, float *lmax) {
    for (int w = DE_THREADS / 2; w > 0; w >>= 1) {
        DE_FOR(l, w) {
            if (lmax[l] < lmax[l + w]) lmax[l] = lmax[l + w];
            if (lmin[l] > lmin[l + w]) lmin[l] = lmin[l + w];
        }
        DE_SYNC();
    }
}

DE_DEV void de_minmax(const DEParams &P, const float *corr, int group, int groups, float *partial, float *lmin, float *lmax) {
    const int total = P.winx * P.winy, step = groups * DE_THREADS;
    DE_FOR(l, DE_THREADS) {
        float lo = corr[0], hi = corr[0];
        for (int t = group * DE_THREADS + l; t < total; t += step) {
            const float cur = corr[t];
            if (hi < cur) hi = cur;
            if (lo > cur) lo = cur;
        }
        lmin[l] = lo; lmax[l] = hi;
    }
    DE_SYNC();
    de_minmax_tree(lmin, lmax);
    DE_FOR(l, 1) { partial[2 * group] = lmin[0]; partial[2 * group + 1] = lmax[0]; }
}

// the same groups paint: (int)((c - min) * norm), norm = pixel_max / (max - min), at (wleft + i, wtop + j) of `plane` (pitch P.pitch), in the clip's
// sample type.  max == min: the reference multiplies 0 by infinity and converts the NaN; here the window becomes 0.
DE_DEV void de_paint(const DEParams &P, const float *corr, const float *partial, int group, int groups, unsigned char *plane, int win, int pixel_max,
                     float *lmin, float *lmax) {
    DE_FOR(l, DE_THREADS) { const int g = l < groups ? l : 0; lmin[l] = partial[2 * g]; lmax[l] = partial[2 * g + 1]; }
    DE_SYNC();
    de_minmax_tree(lmin, lmax);
    const float cmin = lmin[0], cmax = lmax[0];
    const float norm = (float)pixel_max / (cmax - cmin);
    const bool flat = cmax == cmin;
    const int total = P.winx * P.winy, step = groups * DE_THREADS;
    DE_FOR(l, DE_THREADS) {
        for (int t = group * DE_THREADS + l; t < total; t += step) {
            const int i = t & (P.winx - 1), j = t >> P.lgx;
            const int v = flat ? 0 : (int)((corr[t] - cmin) * norm);
            unsigned char *row = plane + (long long)(P.wtop + j) * P.pitch;
            if (P.bits16) ((unsigned short *)row)[P.wleft[win] + i] = (unsigned short)v;
            else row[P.wleft[win] + i] = (unsigned char)v;
        }
    }
}
