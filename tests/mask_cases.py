"""The mv.Mask parity cases, shared by tests/test_mask_host.py (CPU: the condition on the inputs) and tests/test_gpu_mask.py (GPU: byte
equality against tests/mask_ref.py).

A case analyses NF frames of a synthetic clip in one direction, optionally rewrites level 0 of every blob with a recipe of
tests/vector_fields.py, and runs one mv.Mask over all NF frames.  With delta 1 the frame at the clip's end has no reference, so its blob
is Analyse's invalid one: every case mixes usable frames and frames filled with ysc.

The condition on the inputs (POW_MARGIN): the reference calls the C library's pow and truncates 255 * pow(...) to a byte; another pow a few
ULP away (255 has an ULP of 3e-14) gives another byte only where that product lies within a few ULP of an integer.  Every case must keep
every such product at least POW_MARGIN from the integer it must not cross (mask_ref.pow_distance).  Random fields spread the products over
[0, 255), so a case violates it with a probability of about 2 * POW_MARGIN per value; one that does gets another seed, not a tolerance.
The oracle's Analyse (pinned bit-exact to the GPU's by the parity suite) gives the CPU test the vectors the GPU test will see.
"""
import numpy as np

import mask_ref
import pipeline as pl
import vector_fields as vf

POW_MARGIN = 1e-9
NF = 3

FORMATS = {"420": dict(subsampling=(1, 1)), "444": dict(subsampling=(0, 0)), "422": dict(subsampling=(1, 0)), "gray": dict(gray=True, subsampling=(0, 0))}   # a Gray clip has no subsampling: ratios 1 / 1, as mv.Mask requires
R = vf.Recipe
B84, B168, B80 = dict(blksize=8, overlap=4), dict(blksize=16, overlap=8), dict(blksize=8, overlap=0)
B1684 = dict(blksize=16, blksizev=8, overlap=4, overlapv=2)
BW, FW = dict(isb=1), dict(isb=0)
SC = dict(thscd1=20, thscd2=10)   # every analysed frame counts as a scene change

CASES = [
    # fmt, w, h, bits of the analysed clip, super kwargs, analyse kwargs, mask kwargs, recipe, seed, what the restatement's counters must name
    # kind 0: vector length
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=0), None, 201, "sc"),
    ("420", 206, 118, 8, {}, dict(B84, **FW), dict(kind=0, gamma=2.0, ml=3.0, ysc=200), None, 202, "cut,edgex,edgey,sc"),
    ("444", 128, 96, 8, dict(pel=4), dict(B84, **BW), dict(kind=0, gamma=0.5, ml=1000.0), None, 203, "sc"),
    ("422", 160, 96, 8, {}, dict(B80, **FW), dict(kind=0, gamma=0.0), None, 204, "sc"),
    ("gray", 206, 118, 8, dict(pel=1), dict(B84, **BW), dict(kind=0, gamma=0.7, ml=3.0), None, 205, "cut,edgex,edgey,sc"),
    # kind 1: SAD
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=1), None, 211, "sc"),
    ("420", 206, 118, 8, {}, dict(B168, **FW), dict(kind=1, time=0.0, ml=3.0, gamma=0.5), None, 212, "cut,edgex,edgey,sc,trunc"),
    ("422", 160, 96, 8, dict(pel=1), dict(B80, **BW), dict(kind=1, time=37.5, gamma=2.0, ml=1000.0), None, 213, "sc,trunc"),
    ("420", 128, 96, 16, {}, dict(B84, **FW), dict(kind=1, time=37.5), None, 214, "cut,sc,trunc"),                # 16-bit vectors: the SAD is not shifted
    ("gray", 160, 96, 8, {}, dict(B1684, **BW), dict(kind=1, gamma=0.0, ysc=200), None, 215, "edgey,sc"),
    ("444", 128, 96, 8, dict(pel=4), dict(B84, **FW), dict(kind=1, time=0.0, gamma=0.7), None, 216, "moved,sc,trunc"),
    # kind 2: occlusion
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=2), None, 221, "sc"),
    ("420", 206, 118, 8, {}, dict(B84, **FW), dict(kind=2, time=37.5, ml=3.0), None, 222, "cut,edgex,edgey,sc"),
    ("420", 192, 112, 8, {}, dict(B168, **BW), dict(kind=2, gamma=0.5, ml=1000.0), None, 223, "sc"),
    ("444", 128, 96, 8, dict(pel=4), dict(B84, **FW), dict(kind=2, gamma=2.0), None, 224, "sc"),
    ("422", 160, 96, 8, {}, dict(B80, **BW), dict(kind=2, gamma=0.0, time=0.0), None, 225, "cut,sc"),
    ("gray", 160, 96, 8, dict(pel=1), dict(B1684, **FW), dict(kind=2, gamma=0.7, ysc=200), None, 226, "edgey,sc"),
    # kinds 3, 4, 5: the components
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=3), None, 231, "sc"),
    ("420", 206, 118, 8, {}, dict(B84, **FW), dict(kind=3, ml=3.0, ysc=200), None, 232, "cut,edgex,edgey,sc"),
    ("422", 192, 112, 8, {}, dict(B168, **BW), dict(kind=4, ml=1000.0), None, 233, "sc"),
    ("gray", 206, 118, 8, dict(pel=4), dict(B84, **FW), dict(kind=4, ml=3.0), None, 234, "edgex,edgey,sc"),
    ("420", 206, 118, 8, {}, dict(B84, **BW), dict(kind=5), None, 235, "edgex,edgey,sc"),
    ("444", 128, 96, 8, dict(pel=1), dict(B84, **FW), dict(kind=5, ml=3.0), None, 236, "cut,sc"),
    ("422", 160, 96, 8, {}, dict(B1684, **BW), dict(kind=5, ysc=200), None, 237, "edgey,sc"),
    ("gray", 128, 96, 8, {}, dict(B84, **FW), dict(kind=5, ml=1000.0), None, 238, "sc"),
    # 4/2 blocks: one chroma sample per cell, the upsizer's general form (no 8-cell window holds half a segment)
    ("420", 128, 96, 8, {}, dict(blksize=4, overlap=2, isb=1), dict(kind=0, ml=10.0), None, 239, "sc"),
    ("420", 206, 118, 8, {}, dict(blksize=4, overlap=2, isb=0), dict(kind=5, ml=3.0, ysc=200), None, 240, "cut,sc"),
    # a forced scene change: no frame is usable
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=0, ysc=200, **SC), None, 241, "sc"),
    ("420", 206, 118, 8, {}, dict(B84, **FW), dict(kind=5, ysc=200, **SC), None, 242, "sc"),
    # crafted fields
    ("420", 206, 118, 8, {}, dict(B84, **BW), dict(kind=0), R("limits", 1201), 251, "cut,edgex,edgey,sc"),
    ("420", 206, 118, 8, {}, dict(B84, **FW), dict(kind=0, gamma=0.7), R("limits", 1211), 252, "cut,edgex,edgey,sc"),
    ("420", 206, 118, 8, {}, dict(B84, **BW), dict(kind=1, time=0.0, ml=20.0), R("limits", 1221, sad="scd"), 253, "back,cut,edgex,edgey,moved,sc,trunc"),
    ("422", 160, 96, 8, dict(pel=1), dict(B80, **FW), dict(kind=1, time=37.5, gamma=0.5, ml=20.0), R("limits", 1231, sad="scd"), 254, "back,cut,moved,sc,trunc"),
    ("420", 206, 118, 8, {}, dict(B84, **BW), dict(kind=2, gamma=0.7), R("limits", 1241), 255, "cut,edgex,edgey,sc,span"),
    ("444", 128, 96, 8, dict(pel=4), dict(B84, **BW), dict(kind=3), R("limits", 1251), 256, "cut,sc"),
    ("420", 206, 118, 8, {}, dict(B168, **FW), dict(kind=5, ml=3.0), R("limits", 1261), 257, "cut,edgex,edgey,sc"),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=1), R("sad_edges", 1271), 258, "cut,sc"),           # SADs above 2^32
    ("420", 128, 96, 16, {}, dict(B84, **FW), dict(kind=1, gamma=0.5, time=37.5), R("sad_edges", 1281), 259, "cut,sc,trunc"),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=2), R("occlusion", 1291), 260, "cut,sc,span"),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=2, gamma=2.0, time=62.5), R("occlusion", 1301), 261, "cut,sc,span"),
    ("420", 128, 96, 8, {}, dict(B84, **FW), dict(kind=2, time=62.5), R("occlusion", 1305), 265, "cut,sc"),   # a forward range never exceeds two blocks
    ("420", 206, 118, 8, {}, dict(B84, **BW), dict(kind=0), R("scene_count", 1311), 262, "edgex,edgey,sc"),  # count == thscd2: usable
    ("420", 206, 118, 8, {}, dict(B84, **FW), dict(kind=0, ysc=200), R("scene_count", 1321, over=1, only=(1,)), 263, "edgex,edgey,sc"),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(kind=2, ysc=200), R("invalid", 1331, only=(0,)), 264, "sc"),
]
# the benchmarked launch shape
FULL_CASES = [
    ("420", 1920, 1080, 8, {}, dict(B84, **BW), dict(kind=0), None, 271, "sc"),                                # the grid covers the frame
    ("420", 1920, 1080, 8, {}, dict(blksize=32, overlap=0, isb=0), dict(kind=5, ml=3.0), None, 272, "cut,edgey,sc"),   # 33 block rows cover 1056 of 1080
]

ids = lambda cases: ["%d-%s-k%d%s" % (c[8], c[0], c[6]["kind"], "-%r" % c[7] if c[7] else "") for c in cases]


def nf_of(case):
    """frames per case: NF, two at full size"""
    return 2 if case[1] >= 1920 else NF


def time256(mkw):
    return int(mkw.get("time", 100.0) * 256 / 100)


def frames_of(case):
    """the analysed clip (fmt, bits as listed) and, for kind 5, the 8-bit luma planes of the clip argument"""
    fmt, w, h, bits, _, _, mkw, _, seed, _ = case
    f, nf = FORMATS[fmt], nf_of(case)
    frames = pl.moving_clip(w, h, bits, nf, seed=seed, noise=3, sub=f.get("subsampling", (1, 1)))
    if f.get("gray"):
        frames = [[fr[0]] for fr in frames]
    lumas = None
    if mkw["kind"] == 5:
        lumas = [fr[0] for fr in pl.moving_clip(w, h, 8, nf, seed=seed + 1, noise=3)]
    return frames, lumas


def reference_frame(n, isb, nf):
    k = n + 1 if isb else n - 1
    return k if 0 <= k < nf else None


def editor(case, ad):
    """edit(blob, index) of the case's recipe, or the identity.  The occlusion recipe sizes its steps for `256 - time256` of a backward
    blob; mv.Mask uses time256 itself in either direction, so a backward clip passes the complement."""
    mkw, recipe = case[6], case[7]
    if recipe is None:
        return lambda blob, index: np.array(blob, np.uint8, copy=True)
    t = time256(mkw)
    divider = 1.0 / float(np.float32(1.0) / np.float32(mkw.get("ml", 100.0)))   # dMaskNormDivider as mv.Mask forms it (MVMask.c:145,304)
    e = recipe.editor(thscd1=mkw.get("thscd1", 400), thscd2=mkw.get("thscd2", 130), ml=divider, time256=256 - t if ad.isBackward else t)
    return lambda blob, index: e(np.asarray(blob, np.uint8), ad, index)


def oracle_vectors(oracle, case):
    """(analysis data, the edited blobs of frames 0 .. nf - 1) through the CPU oracle"""
    fmt, w, h, bits, skw, akw, _, _, _, _ = case
    frames, _ = frames_of(case)
    nf = nf_of(case)
    sup = oracle.Super(w, h, bits, **dict(FORMATS[fmt], **skw))
    sf = [sup.frame(fr) for fr in frames]
    an = oracle.Analyse(sup, num_frames=nf, **akw)
    edit = editor(case, an.ad)
    blobs = []
    for n in range(nf):
        k = reference_frame(n, akw["isb"], nf)
        blobs.append(edit(an.frame(sf[n], sf[k] if k is not None else None), n))
    return an.ad, blobs


def expected(case, ad, blobs, lumas):
    """the restatement over the case's frames: (frames of three planes, the counters that fired as a sorted string, pow_dist)"""
    ref = mask_ref.Mask(ad, **case[6])
    stats = {}
    want = [ref.frame(b, lumas[n] if lumas is not None else None, stats) for n, b in enumerate(blobs)]
    return want, ",".join(sorted(k for k, v in stats.items() if v > 0)), ref.pow_dist
