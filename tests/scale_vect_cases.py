"""The cases of ScaleVect shared by tests/test_scale_vect_host.py (the analysis data, on the CPU) and tests/test_gpu_scale_vect.py (the blobs
and what the consumers make of them, on the GPU).  Test infrastructure.

A case: the small clip the vectors are searched on, the scale, and the target super clip the scaled vectors are used on."""
import collections

import vector_fields as vf

Case = collections.namedtuple("Case", "name fmt w h bits pel scale tbits tpel tpad akw edit inplace")

SUB = {"420": dict(subsampling=(1, 1)), "422": dict(subsampling=(1, 0)), "444": dict(subsampling=(0, 0)), "gray": dict(gray=True)}

B84, B42 = dict(blksize=8, overlap=4), dict(blksize=4, overlap=2)
B8442 = dict(blksize=8, blksizev=4, overlap=4, overlapv=2)


def _c(name, fmt="420", w=96, h=64, bits=8, pel=2, scale=2, tbits=8, tpel=2, tpad=32, akw=B84, edit=None, inplace=False):
    return Case(name, fmt, w, h, bits, pel, scale, tbits, tpel, tpad, akw, edit, inplace)


# edit: None = the vectors Analyse found; "limits" = vector_fields.limits on the small blob (every block on or inside its legal rectangle on
# the SMALL super clip, whose padding is 16) with one SAD_HIGH and a long vector on the coarsest level; "invalid" = the validity word cleared
CASES = [
    # shapes: 96x64 -> 192x128 at 2 (8x8/4 -> 16x16/8 and 8x4 -> 16x8), 48x32 -> 192x128 at 4 (4x4/2 -> 16x16/8), an uncovered strip
    _c("420-8to8-16x16"),
    _c("420-8to8-16x8", akw=B8442),
    _c("420-8to8-scale4", w=48, h=32, scale=4, tpad=64, akw=B42),
    _c("420-8to8-strip", w=100, h=68),
    # depths
    _c("420-8to16", tbits=16),
    _c("420-16to8", bits=16),
    _c("420-8to16-scale1", scale=1, tbits=16, tpad=16),
    # formats
    _c("422-8to8", fmt="422"),
    _c("444-8to16", fmt="444", tbits=16),
    _c("gray-8to8", fmt="gray"),
    # pel pairs: 2 -> 2 is every case above (m = 2); 2 -> 1 (m = 1); 1 -> 2 (m = 4)
    _c("420-pel2to1", tpel=1),
    _c("420-pel1to2", pel=1),
    # the clamp: target padding 32 = twice the small clip's (the identity) and 16 (blocks clamp on all four sides)
    _c("420-limits-pad32", edit="limits"),
    _c("420-limits-pad16", tpad=16, edit="limits"),
    _c("420-limits-pad16-8to16-pel1to2", pel=1, tbits=16, tpad=16, edit="limits"),
    _c("420-limits-pad16-scale4", w=48, h=32, scale=4, tpad=16, akw=B42, edit="limits"),
    _c("420-limits-pad16-16to8", bits=16, tpad=16, edit="limits"),
    # an invalid blob, a SAD above 2^32 (in "limits"), in place
    _c("420-invalid", edit="invalid"),
    _c("420-inplace", tbits=16, tpad=16, edit="limits", inplace=True),
]

MULTI = _c("420-multi-radius2", tbits=16, tpad=16, edit="limits")   # a multi blob of radius 2 in one call


def super_kwargs(case, target):
    kw = dict(SUB[case.fmt])
    if target:
        kw.update(pel=case.tpel, hpad=case.tpad, vpad=case.tpad)
    else:
        kw.update(pel=case.pel)
    return kw


def sizes(case):
    return (case.w, case.h), (case.scale * case.w, case.scale * case.h)


def target_analyse_kwargs(case):
    """Analyse's arguments on the target super clip that give the scaled clip's analysis data"""
    return {k: v * case.scale for k, v in case.akw.items()}


def smaller_blocks(case):
    """Recalculate's arguments at full size: half the scaled block size"""
    kw = {k: v * case.scale // 2 for k, v in case.akw.items()}
    return dict(kw, thsad=100)


PAN = (4, 2)   # pixels per frame of the end-to-end clip at full size; (2, 1) on its 2x2 box mean


def pan_clips(w, h, nframes, seed=5):
    """(full, small): a w x h 8-bit 4:2:0 texture whose content moves by PAN per frame, and its 2x2 box mean.  PAN is even, so the small
    clip is the same texture at half size moving by exactly PAN / 2: the search has an exact match at (2, 1) pixels.  Chroma is flat (a pan
    of half a chroma sample is no pan of the box mean)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    bw, bh = w + PAN[0] * nframes + 8, h + PAN[1] * nframes + 8
    coarse = rng.integers(0, 256, (bh // 4 + 2, bw // 4 + 2)).astype(np.float64)
    tex = np.kron(coarse, np.ones((4, 4)))[:bh, :bw]                      # 4 x 4 cells: two samples of the small clip each way
    tex = (tex + np.roll(tex, 1, 0) + np.roll(tex, 1, 1) + np.roll(tex, (1, 1), (0, 1))) / 4 + rng.integers(-6, 7, (bh, bw))
    tex = np.clip(np.rint(tex), 0, 255).astype(np.uint8)
    full, small = [], []
    for f in range(nframes):
        oy, ox = PAN[1] * (nframes - f), PAN[0] * (nframes - f)          # content moves right and down
        y = tex[oy:oy + h, ox:ox + w]
        ys = ((y[0::2, 0::2].astype(np.int32) + y[0::2, 1::2] + y[1::2, 0::2] + y[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        full.append([y.copy(), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)])
        small.append([ys, np.full((h // 4, w // 4), 128, np.uint8), np.full((h // 4, w // 4), 128, np.uint8)])
    return full, small


def interior(a):
    """the blocks of a level-0 array that touch no frame edge"""
    return a[1:-1, 1:-1]


def edit_small(case, blob, ad, index):
    """the edited copy of a blob of the small clip"""
    if case.edit is None:
        return vf._fresh(blob)
    if case.edit == "invalid":
        return vf.invalid(blob, ad)
    b = vf.limits(blob, ad, 7001 + index)
    _, sad = vf.records(b, ad)
    sad[0, 0] = sad[-1, -1] = vf.SAD_HIGH
    if ad.nLvCount > 1:                               # the coarser levels are scaled and NOT clamped; no consumer reads them
        xy, csad = vf.records(b, ad, 1)
        xy[0, 0, 0], xy[0, 0, 1], csad[0, 0] = 100000, -100000, vf.SAD_HIGH
        xy[-1, -1, 0], xy[-1, -1, 1], csad[-1, -1] = -2 ** 30, 2 ** 30, -3   # x * m leaves 32 bits at m = 4; a negative SAD: the arithmetic shift
    return b
