// mvx_depan_stab_sample.h -- DepanStabilise's selection for one output sample, on top of the unchanged interpolators of mvx_depan_sample.h:
// what depan_stab_kernel of mvx_depan_stab.hip runs per thread.  A header without HIP, so that tests/test_depan_stab_ref.py compiles the
// same text for the host.  Build with -ffp-contract=off.
//
// The reference paints one destination up to three times (MVDepan.cpp:3679-3693): fillBorderPrev (nearest, the filter's mirror, the border
// value), fillBorderNext (nearest; border -1 and no mirror once prev has painted), compensateFrame (the subpixel interpolator; border -1 and
// no mirror once anything has painted).  A pass with border -1 leaves a sample alone where its position is outside its source, and every
// pass writes a pure function of its own source, so the last pass that holds a sample decides it: the current frame, else next, else prev.
// A plane's three sources lie side by side, S[DS_CUR], S[DS_NEXT], S[DS_PREV]; an unused one has src == nullptr.  Exactly the first pass
// painted carries a border value >= 0 and the mirror bits, so the selection always ends on a value >= 0.
#pragma once
#include "mvx_depan_sample.h"

enum { DS_CUR = 0, DS_NEXT = 1, DS_PREV = 2, DS_SOURCES = 3 };

// (host) the plane's transform and its form from the pass's luma transform, MVDepan.cpp:3366-3379 (the rule of :2687-2700 and of
// dc_plane_transform in mvx_depan.hip); tr: dxc dxx dxy dyc dyx dyy
static inline void ds_plane_transform(int ssw, int ssh, int p, const float *tr, DCPlane *P) {
    float dxc = tr[0], dxx = tr[1], dxy = tr[2], dyc = tr[3], dyx = tr[4], dyy = tr[5];
    if (p && ssw == 1 && ssh == 1) { dxc /= 2; dyc /= 2; }
    else if (p && ssw == 1 && ssh == 0) { dxc /= 2; dxy /= 2; dyx *= 2; }
    P->dxc = dxc; P->dxx = dxx; P->dxy = dxy; P->dyc = dyc; P->dyx = dyx; P->dyy = dyy;
    P->cls = (dxy == 0.0f && dyx == 0.0f && dxx == 1.0f && dyy == 1.0f) ? 0 : (dxy == 0.0f && dyx == 0.0f) ? 1 : 2;
}

// (host) border values of the passes of one plane: `border` for the first pass painted (prev, else next, else the current frame), -1 for the others
static inline void ds_borders(DCPlane *S, int border) {
    S[DS_PREV].border = border;
    S[DS_NEXT].border = S[DS_PREV].src ? -1 : border;
    S[DS_CUR].border = S[DS_PREV].src || S[DS_NEXT].src ? -1 : border;
}

template <typename T, int SUB> DC_FN int ds_sample(const DCPlane *S, const DCCommon &C, int h, int row) {
    const DCCommon none = { 0, C.pixel_max, C.nplanes };
    int v = SUB == 0 ? dc_nearest<T>(S[DS_CUR], S[DS_CUR].border >= 0 ? C : none, h, row)
          : SUB == 1 ? dc_bilinear<T>(S[DS_CUR], S[DS_CUR].border >= 0 ? C : none, h, row)
                     : dc_bicubic<T>(S[DS_CUR], S[DS_CUR].border >= 0 ? C : none, h, row);
    if (v < 0 && S[DS_NEXT].src) v = dc_nearest<T>(S[DS_NEXT], S[DS_NEXT].border >= 0 ? C : none, h, row);
    if (v < 0 && S[DS_PREV].src) v = dc_nearest<T>(S[DS_PREV], C, h, row);
    return v;
}
