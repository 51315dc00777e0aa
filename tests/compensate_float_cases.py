"""What the float Compensate / CompensateN tests share (test infrastructure): the GPU cases with their thsad, the restatement set up from a
filter's arguments, the error bound against the integer filter, and crafted fields that still fall back on some blocks.

The searched cases run on tests/multi_cases.py's clip (96x64, 2 * tr + 3 frames, every frame a job) and on two small sizes; the float clip is
degrain_float_cases.float_clip of the integer clip, whose quantised copy is the integer clip itself, so the search -- and with it the shares of
compensated blocks -- is the integer clip's.  tests/test_compensate_float_cases.py shows through the oracle that every case's thsad leaves at
least multi_cases.USED of the (block, field) pairs compensated and at least multi_cases.UNUSED not."""
import numpy as np

import compensate_float_ref
import multi_cases as mc
import vector_fields

B168P4 = ("p4b16", dict(pel=4), dict(blksize=16, overlap=8))   # 11 x 7 blocks; cells of 4 / 4 samples, sixteen sub-pel planes
B84P0 = ("p2pad0", dict(pel=2, hpad=0, vpad=0), dict(blksize=8, overlap=4))
B42P1 = ("p1b4", dict(pel=1), dict(blksize=4, overlap=2))

# (fmt, bits of the searched copy, (tag, super kwargs, analyse kwargs), tr, w, h, thsad).  The 96x64 geometries of tests/multi_cases.py keep its
# THSAD (tests/test_multi_cases.py has shown the shares); the others were chosen on the CPU with tests/test_compensate_float_cases.py
W, H = mc.W, mc.H
SEARCHED = [
    ("420", 16, mc.B84, 1, W, H, mc.THSAD),      # cells of 4 and 2
    ("420", 16, mc.B84, 3, W, H, mc.THSAD),
    ("420", 16, mc.B84, 7, W, H, mc.THSAD),
    ("420", 8, mc.B84, 3, W, H, mc.THSAD),       # the search on the 8-bit copy
    ("420", 16, mc.B42, 3, W, H, mc.THSAD),      # chroma cells of one sample
    ("420", 8, mc.B42, 1, W, H, mc.THSAD),
    ("420", 16, mc.B160, 3, W, H, mc.THSAD),     # blocks side by side, pel 1
    ("420", 8, mc.B160, 7, W, H, mc.THSAD),
    ("444", 8, mc.B84, 3, W, H, mc.THSAD),
    ("gray", 8, mc.B160, 3, W, H, mc.THSAD),
    ("420", 16, B168P4, 3, W, H, 400),           # pel 4
    ("420", 8, B168P4, 1, W, H, 400),
    ("420", 16, mc.B84, 2, 70, 54, 300),         # chroma 35 x 27: cells cut by the edge, strips no block covers
    ("420", 16, mc.B160, 2, 70, 54, 300),
    ("420", 8, B42P1, 1, 70, 54, 300),
    ("gray", 16, B84P0, 2, 36, 36, 300),         # no padding
]


def case_id(c):
    fmt, bits, blk, tr, w, h, thsad = c
    return "%dx%d-%s-%dbit-blk%d-ov%d-%s-tr%d" % (w, h, fmt, bits, blk[2]["blksize"], blk[2]["overlap"], blk[0], tr)


def restatement(oracle, ad, ckw, gray=False):
    """tests/compensate_float_ref.py for a filter created with the keyword arguments ckw on vectors of analysis data ad"""
    th, s1, s2 = vector_fields.scaled_thresholds(ad, ckw.get("thsad", 10000), ckw.get("thscd1", 400), ckw.get("thscd2", 130))
    return compensate_float_ref.CompensateFloat(oracle, ad, th, s1, s2, time=ckw.get("time", 100.0), scbehavior=ckw.get("scbehavior"), gray=gray)


def bound(peak):
    """|float - integer| for overlapped blocks on integer-valued samples up to peak; tests/test_compensate_float_ref.py derives it"""
    return 0.625 + peak / 2048.0 + 5 * peak * (2049.0 / 2048.0) * 2.0 ** -24 * (1 + 2.0 ** -20)


def with_fallbacks(blob, ad, seed, thsad, share=0.1):
    """vector_fields.limits, and then `share` of the blocks (one at least) with a SAD on the scaled thsad: they fall back on the source block"""
    b = vector_fields.limits(blob, ad, seed)
    _, sad = vector_fields.records(b, ad)
    th = vector_fields.scaled_thresholds(ad, thsad)[0]
    count = max(1, int(round(share * sad.size)))  # (a grid of a dozen blocks still gets one)
    pick = np.zeros(sad.size, bool)
    pick[np.random.default_rng(seed + 1000).choice(sad.size, count, replace=False)] = True
    sad[pick.reshape(sad.shape)] = th
    assert 0 < count < sad.size // 2
    return b
