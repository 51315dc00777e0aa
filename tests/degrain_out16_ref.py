"""The yardstick of mv.DegrainN's out16 (test infrastructure): NOT a third statement of the arithmetic, but the 16-bit path of the
restatement that tests/test_degrain_n_ref.py holds to the oracle (tests/degrain_n_ref.py), fed what the definition names
(include/mvtools_amd.h, mvx_degrain_n_create_out16):

    the analysis data with bitsPerSample 16          -> its 16-bit arithmetic: 32-bit accumulator, clamp and limits at 65535
    the 8-bit filter's own threshold tables (info())  \\  the weights of the 8-bit run: SADs, thresholds and scene-change thresholds
    the 8-bit scene-change thresholds                 /  stay in 8-bit units
    source and super planes shifted left by 8, uint16
    limit / limitc in units of the output

A block's value there is (128 + 256 * S) >> 8 = S, the sum the 8-bit kernel forms before it drops eight bits."""
import numpy as np

import degrain_n_ref
import vector_fields


def widen(planes):
    """8-bit planes -> the same samples shifted left by 8, uint16; None stays None"""
    if planes is None:
        return None
    for p in planes:
        assert np.asarray(p).dtype == np.uint8
    return [np.asarray(p).astype(np.uint16) << 8 for p in planes]


def restatement(oracle, radius, ad, th_luma, th_chroma, dkw, gray=False):
    """ad: the 8-bit vector clips' analysis data; th_luma / th_chroma: the 8-bit filter's scaled thresholds per distance; dkw: the
    filter's other arguments (limit / limitc in output units)"""
    assert ad.bitsPerSample == 8
    _, s1, s2 = vector_fields.scaled_thresholds(ad, 400, dkw.get("thscd1", 400), dkw.get("thscd2", 130))
    ad16 = type(ad).from_buffer_copy(bytes(ad))
    ad16.bitsPerSample = 16
    return degrain_n_ref.DegrainN(oracle, radius, ad16, th_luma, th_chroma, s1, s2, plane=dkw.get("plane", 4), limit=dkw.get("limit"),
                                  limitc=dkw.get("limitc"), gray=gray)


def frame(ref, src, ref_supers, blobs):
    """the out16 planes of one job: 8-bit source planes, 8-bit super frames (or None), the 8-bit search's blobs"""
    return ref.frame(widen(src), [widen(s) for s in ref_supers], blobs)


def window_totals(win, nbx, nby, bw, bh, ox, oy):
    """per sample of the covered area, the sum of the window weights of the blocks that cover it, and the smallest weight: the windows laid
    out as overlaps_c lays them out (MVDegrains.cpp:256-262,285)"""
    stepx, stepy = bw - ox, bh - oy
    total = np.zeros((nby * stepy + oy, nbx * stepx + ox), np.int64)
    for by in range(nby):
        wby = ((by + nby - 3) // (nby - 2)) * 3
        for bx in range(nbx):
            wbx = 2 if bx == nbx - 1 else (0 if bx == 0 else 1)
            total[by * stepy:by * stepy + bh, bx * stepx:bx * stepx + bw] += win[wby + wbx]
    return total, int(win.min())
