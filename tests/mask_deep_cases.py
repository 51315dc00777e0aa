"""The deep mv.Mask parity cases, shared by tests/test_mask_deep_host.py (CPU: the conditions on the inputs) and tests/test_gpu_mask_deep.py
(GPU: sample equality against tests/mask_deep_ref.py).  The form is that of tests/mask_cases.py with the clip's depth appended; the
analysed clip has that depth too, so the SADs of kind 1 are on the scale the shift is made for.

What the cases cover between them (tests/test_mask_deep_host.py asserts it): depths 9, 10, 12, 14 and 16, and 8 through the deep entry; every
kind at gamma 1 and another; 4:2:0, 4:2:2, 4:4:4 and Gray; the three forms of the upsizer (16/8 blocks: one window; 8/4 blocks in 4:2:0: a
window per half in the chroma planes; 4/2 blocks in 4:2:0: the general form); plane widths whose last 16-sample segment holds 16, 14, 9, 8, 7,
2 and 1 samples (luma / chroma: 128 x 96 16 / 16, 206 x 118 14 / 7, 137 x 96 4:4:4 9 / 9, 144 x 96 16 / 8, 130 x 98 2 / 1); plane heights that
leave 0, 1, 2 and 3 rows in the last group of four (96, 49, 98 and 118, 59); a forced scene change and an invalid blob in both expansion forms;
the crafted fields of tests/vector_fields.py.

The conditions: POW_MARGIN of tests/mask_cases.py; the counters each case names; and for every kind 1 case the restatement's `shifted` is at
least half of `cells`, so that a kernel without the shift cannot pass.
"""
import numpy as np

import mask_cases as mc
import mask_deep_ref
import pipeline as pl
import vector_fields as vf

POW_MARGIN = mc.POW_MARGIN
R = vf.Recipe
B84, B168, B80, BW, FW, SC = mc.B84, mc.B168, mc.B80, mc.BW, mc.FW, mc.SC
B42 = dict(blksize=4, overlap=2)

CASES = [
    # fmt, w, h, bits of the analysed clip, super kwargs, analyse kwargs, mask kwargs, recipe, seed, the restatement's counters, the clip's depth
    # kind 1: the shifted SAD
    ("444", 137, 96, 16, {}, dict(B84, **BW), dict(kind=1), None, 301, "edgex,sc", 16),
    ("420", 130, 98, 10, {}, dict(B84, **BW), dict(kind=1, time=37.5), None, 302, "edgex,edgey,sc,trunc", 10),
    ("420", 206, 118, 12, {}, dict(B168, **FW), dict(kind=1, time=0.0, ml=30.0, gamma=0.5), None, 303, "cut,edgex,edgey,sc,trunc", 12),
    ("422", 160, 96, 14, dict(pel=1), dict(B80, **BW), dict(kind=1, gamma=2.0, ml=300.0), None, 304, "sc", 14),
    ("420", 128, 96, 9, {}, dict(B42, **BW), dict(kind=1), None, 305, "sc", 9),
    ("420", 128, 96, 16, {}, dict(B84, **FW), dict(kind=1, gamma=0.5, time=37.5), R("sad_edges", 1281), 306, "cut,sc,trunc", 16),   # SADs above 2^32
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=1), None, 308, "sc", 8),                                                  # the deep entry at 8 bits: no shift
    # kind 0: vector length, a weight
    ("gray", 206, 118, 16, dict(pel=4), dict(B84, **FW), dict(kind=0, gamma=0.7, ml=3.0), None, 307, "cut,edgex,edgey,sc", 16),
    ("420", 144, 96, 10, {}, dict(B84, **BW), dict(kind=0), None, 311, "sc", 10),
    ("420", 130, 98, 14, {}, dict(B168, **FW), dict(kind=0, gamma=2.0, ml=3.0, ysc=200), None, 312, "cut,edgex,edgey,sc", 14),
    # kind 2: occlusion, a weight
    ("420", 206, 118, 12, {}, dict(B84, **FW), dict(kind=2, time=37.5, ml=3.0), None, 313, "cut,edgex,edgey,sc", 12),
    ("gray", 128, 96, 9, {}, dict(B84, **BW), dict(kind=2, gamma=0.5, ml=1000.0), None, 318, "sc", 9),
    ("420", 144, 96, 14, {}, dict(B168, **BW), dict(kind=2, gamma=2.0), None, 320, "sc", 14),
    # kinds 3, 4, 5: the components, offsets from the neutral value
    ("420", 130, 98, 16, {}, dict(B84, **BW), dict(kind=3, ml=3.0, ysc=200), None, 314, "edgex,edgey,sc", 16),
    ("422", 160, 96, 14, {}, dict(B168, **FW), dict(kind=4), None, 315, "sc", 14),
    ("420", 206, 118, 10, {}, dict(B84, **BW), dict(kind=5), None, 316, "edgex,edgey,sc", 10),
    ("444", 137, 96, 12, dict(pel=1), dict(B84, **FW), dict(kind=5, ml=3.0), None, 317, "cut,edgex,sc", 12),
    ("420", 128, 96, 16, {}, dict(B42, **FW), dict(kind=5, ml=3.0, ysc=200), None, 319, "cut,sc", 16),                           # the general form, two bytes a sample
    ("420", 206, 118, 8, {}, dict(B84, **FW), dict(kind=5), None, 339, "edgex,edgey,sc", 8),                                     # the deep entry at 8 bits
    # a forced scene change: no frame is usable; E(ysc) in both forms
    ("420", 128, 96, 16, {}, dict(B84, **BW), dict(kind=0, ysc=200, **SC), None, 321, "sc", 16),
    ("420", 206, 118, 10, {}, dict(B84, **FW), dict(kind=5, ysc=200, **SC), None, 322, "sc", 10),
    # crafted fields
    ("420", 206, 118, 16, {}, dict(B84, **BW), dict(kind=0), R("limits", 1201), 331, "cut,edgex,edgey,sc", 16),
    ("444", 137, 96, 12, dict(pel=4), dict(B84, **BW), dict(kind=3), R("limits", 1251), 332, "cut,edgex,sc", 12),
    ("420", 130, 98, 10, {}, dict(B168, **FW), dict(kind=5, ml=3.0), R("limits", 1261), 333, "cut,edgex,edgey,sc", 10),
    ("420", 128, 96, 16, {}, dict(B84, **BW), dict(kind=2), R("occlusion", 1291), 334, "cut,sc,span", 16),
    ("420", 206, 118, 12, {}, dict(B84, **FW), dict(kind=0, ysc=200), R("scene_count", 1321, over=1, only=(1,)), 335, "edgex,edgey,sc", 12),
    ("420", 128, 96, 14, {}, dict(B84, **BW), dict(kind=2, ysc=200), R("invalid", 1331, only=(0,)), 336, "sc", 14),              # E(ysc) of a weight
    ("420", 130, 98, 9, {}, dict(B84, **BW), dict(kind=3, ysc=77), R("invalid", 1341, only=(1,)), 337, "edgex,edgey,sc", 9),     # E(ysc) of an offset
]
# the benchmarked launch shape
FULL_CASES = [
    ("420", 1920, 1080, 16, {}, dict(B84, **BW), dict(kind=0), None, 371, "sc", 16),
]
# depth independence of kind 1: format, size, analyse kwargs, depth (pel 1: no interpolation, so the SADs of the shifted clip are exact multiples)
INDEPENDENCE = [("420", 128, 96, B84, 16), ("420", 206, 118, B168, 12), ("422", 160, 96, B80, 10)]

ids = lambda cases: ["%d-%s-k%d-b%d%s" % (c[8], c[0], c[6]["kind"], c[10], "-%r" % c[7] if c[7] else "") for c in cases]


def frames_of(case):
    """the analysed clip and, for kind 5, the luma planes of the clip argument at the clip's depth"""
    fmt, w, h, _, _, _, mkw, _, seed, _, depth = case
    frames, _ = mc.frames_of(case[:10])
    lumas = None
    if mkw["kind"] == 5:
        lumas = [fr[0] for fr in pl.moving_clip(w, h, depth, mc.nf_of(case), seed=seed + 1, noise=3)]
    return frames, lumas


def oracle_vectors(oracle, case):
    return mc.oracle_vectors(oracle, case[:10])


def expected(case, ad, blobs, lumas):
    """the restatement over the case's frames: (frames of three planes, the counters that fired as a sorted string, the restatement itself)"""
    ref = mask_deep_ref.DeepMask(ad, case[10], **case[6])
    stats = {}
    want = [ref.frame(b, lumas[n] if lumas is not None else None, stats) for n, b in enumerate(blobs)]
    return want, ",".join(sorted(k for k, v in stats.items() if v > 0)), ref


def independence_clips(geo):
    """the NF frames of an 8-bit clip and the same frames with every sample shifted left by depth - 8 (frame 0 is analysed against frame 1)"""
    fmt, w, h, _, depth = geo
    low = pl.moving_clip(w, h, 8, mc.NF, seed=77, noise=3, sub=mc.FORMATS[fmt]["subsampling"])
    return low, [[(p.astype(np.uint16) << (depth - 8)) for p in fr] for fr in low]
