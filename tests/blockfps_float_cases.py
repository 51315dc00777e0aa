"""What the float BlockFPS tests share (test infrastructure): the geometries and cases of tests/test_gpu_blockfps_float.py, the clip with the two
vector clips of every frame, the restatement set up from a filter's arguments, the jobs of an output frame, the mask shares a case must reach
and the error bound against the integer filter.

The float clip is degrain_float_cases.float_clip of the integer clip, whose quantised copy is the integer clip itself, so the search -- and with
it the masks -- is the integer clip's.  tests/test_blockfps_float_cases.py shows through the oracle's search that every masked case's ml leaves a
mask that is neither empty nor saturated."""
import numpy as np

import blockfps_float_ref
import degrain_n_cases as dc
import multi_cases as mc
import vector_fields

F = np.float32
NFRAMES = 5                       # 24 -> 60 over five input frames: eleven output frames
SHARE = 0.1                       # of the luma samples of a masked case: a mask above 0, and a mask below 255

B84, B160, B42 = mc.B84, mc.B160, mc.B42
B168P4 = ("p4b16", dict(pel=4), dict(blksize=16, overlap=8))
B84P0 = ("p2pad0", dict(pel=2, hpad=0, vpad=0), dict(blksize=8, overlap=4))
B42P1 = ("p1b4", dict(pel=1), dict(blksize=4, overlap=2))
SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "gray": (1, 1)}

# (fmt, bits of the searched copy, (tag, super kwargs, analyse kwargs), w, h, mode, ml).  The vectors are searched; ml per case was chosen on the
# CPU with tests/test_blockfps_float_cases.py (modes 0..2 read no mask and keep the default).  The searched fields are too smooth for the
# occlusion masks of modes 3..5 -- under a tenth of the samples at any ml -- so those modes run on crafted fields (MODES, SMALL)
SEARCHED = [
    ("420", 16, B84, 96, 64, 6, 20.0),        # cells of 4 and 2
    ("420", 8, B84, 96, 64, 8, 20.0),         # the search on the 8-bit copy
    ("420", 8, B42, 96, 64, 7, 20.0),         # chroma cells of one sample
    ("420", 16, B160, 96, 64, 8, 20.0),       # blocks side by side, pel 1
    ("420", 8, B168P4, 96, 64, 7, 20.0),      # pel 4
    ("420", 16, B84, 70, 54, 7, 20.0),        # chroma 35 x 27: cells cut by the edge, strips no block covers
    ("420", 16, B160, 70, 54, 1, 100.0),
    ("gray", 16, B84P0, 36, 36, 6, 20.0),     # no padding
    ("444", 8, B84, 96, 64, 7, 60.0),         # (full-size chroma: larger SADs)
    ("422", 16, B160, 96, 64, 6, 20.0),
]
# all nine modes on one overlapped and one side-by-side geometry, on crafted fields: (fmt, bits, blk, w, h, recipe); ml is crafted_ml's
MODES = [("420", 16, B84, 96, 64, "occlusion"), ("420", 8, B160, 96, 64, "limits")]
SMALL = [("420", 16, B84, 70, 54), ("420", 16, B160, 70, 54), ("420", 8, B42P1, 70, 54), ("gray", 16, B84P0, 36, 36)]


def geo_id(fmt, bits, blk, w, h):
    return "%dx%d-%s-%dbit-blk%d-ov%d-%s" % (w, h, fmt, bits, blk[2]["blksize"], blk[2]["overlap"], blk[0])


def searched_id(c):
    return "%s-mode%d" % (geo_id(*c[:5]), c[5])


def int_clip(fmt, bits, w, h, n=NFRAMES):
    return dc.clip(w, h, bits, n, fmt)


def vector_jobs(n):
    """per input frame its reference for mvbw (delta 1) and for mvfw, None outside the clip"""
    return [m + 1 if m + 1 < n else None for m in range(n)], [m - 1 if m >= 1 else None for m in range(n)]


def restatement(oracle, ad_bw, ad_fw, bkw, gray=False):
    """tests/blockfps_float_ref.py for a filter created with the keyword arguments bkw"""
    _, s1, s2 = vector_fields.scaled_thresholds(ad_bw, 400, bkw.get("thscd1", 400), bkw.get("thscd2", 130))
    return blockfps_float_ref.BlockFPSFloat(oracle, ad_bw, ad_fw, s1, s2, mode=bkw.get("mode"), ml=bkw.get("ml", 100.0), blend=bkw.get("blend"), gray=gray)


def want_frame(ref, fmap, n, clip, sups, blobs_bw, blobs_fw):
    """output frame n of a clip of len(clip) frames as the package's BlockFPS.run sets the job up: fmap(n) -> (nleft, nright, time256)"""
    nl, nr, t = fmap(n)
    last = len(clip) - 1
    good = nl <= last and nr <= last
    return ref.frame(t, clip[min(nl, last)], clip[min(nr, last)], sups[nl] if good else None, sups[nr] if good else None,
                     blobs_fw[nr] if good else None, blobs_bw[nl] if good else None)


def mask_shares(ref):
    """after a usable frame in a mask mode: over the masks the mode reads, the smallest share of luma samples above 0 and below 255"""
    F_, B_, O_ = ref.masks
    read = [O_] if ref.mode in (5, 8) else [F_, B_] if ref.mode in (3, 6) else [F_, B_, O_]
    return min(float((m > 0).mean()) for m in read), min(float((m < 255).mean()) for m in read)


def crafted_ml(recipe, mode):
    """the ml at which a crafted field's masks are neither empty nor saturated: the occlusion profile is sized for the default; vectors on the
    limits differ by hundreds of sub-pel steps, so their occlusion needs a large divider; SADs up to thscd1 reach 255 at about ml 25"""
    return 40.0 if mode >= 6 else 100.0 if recipe == "occlusion" else 2000.0


def crafted(recipe, blob, ad, seed, bkw, t=128):
    """a level-0 field for a mask mode: vector_fields' occlusion profile (grids of 14 x 14 blocks and more) or vectors on the limits of their legal
    rectangles; SADs up to thscd1 so that the SAD masks of modes 6..8 are not empty"""
    r = vector_fields.Recipe(recipe, seed, sad="scd", **(dict(time256=t) if recipe == "occlusion" else {}))
    return vector_fields.case_editor("blockfps", r, bkw)(blob, ad, 0)


# ---- |float - integer| on integer-valued samples 0..peak; tests/test_blockfps_float_ref.py derives it
D = 255.0 / 256.0   # what one "(... + 255) >> 8" against "/ 255", or one ">> 8" against "* K", can differ by


def bound(mode, overlap, peak):
    stages = {0: 1, 1: 1, 2: 1, 3: 2, 6: 2, 4: 3, 7: 3}[mode]
    ops = {0: 0, 1: 0, 2: 0, 3: 11, 6: 11, 4: 18, 7: 18}[mode]
    assert peak == 255 or mode < 3, "the mask mixes are 8-bit arithmetic: compared on samples 0..255 only"
    b = stages * D + ops * peak * (256.0 / 255.0) * 2.0 ** -24
    if overlap:
        b += 0.625 + peak / 2048.0 + 5 * peak * (2049.0 / 2048.0) * 2.0 ** -24
    return b * (1 + 2.0 ** -20)
