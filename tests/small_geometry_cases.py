"""What the tests of the search on tiny and unpadded clips share (test infrastructure): the geometries, the clips, and the list of kernel
routes a geometry can take.

A level of a super clip made with a padding below the chroma ratio is FLOORED (MVFrame.cpp:1209-1226), the block grid of mv.Analyse is not
(nWidth_B >> level): on the coarsest levels of a small clip a block can stick out of its level, its legal rectangle is EMPTY
(nDxMax <= nDxMin), and the clip min(max(v, nDxMin), nDxMax - 1) sends the zero / global / hierarchical predictors a sample or a few to the
left of and above the level's first sample -- which the reference and the oracle load without asking whether the vector is legal.
tests/test_search_addressing.py audits the kernels' 32-bit offsets there on the CPU, tests/test_gpu_small_geometry.py runs them."""
import itertools

import numpy as np

import pipeline as pl

SUB = {"gray": (1, 1), "420": (1, 1), "444": (0, 0)}
BLOCKS = [(8, 4), (8, 0), (16, 8), (16, 0), (32, 16)]
PADS = [(0, 0), (1, 1), (2, 0)]


def geometry(w, h, fmt, bits, pel, pad, blk, shadow=True, levels=None, **akw):
    skw = dict(pel=pel, hpad=pad[0], vpad=pad[1])
    a = dict(blksize=blk[0], overlap=blk[1])
    if levels:
        skw["levels"] = levels
        a["levels"] = levels
    a.update(akw)
    name = "%dx%d-%s-%dbit-pel%d-pad%d.%d-blk%d.%d%s%s" % (w, h, fmt, bits, pel, pad[0], pad[1], blk[0], blk[1], "" if shadow else "-noshadow", "-lv%d" % levels if levels else "") + ("-pelsearch%d" % akw["pelsearch"] if "pelsearch" in akw else "")
    return dict(name=name, w=w, h=h, fmt=fmt, bits=bits, skw=skw, akw=a, shadow=shadow)


# the search that faulted on a GPU (profiles/flow_float_gpu_suite.txt): 8-bit, 36x36, Gray, no padding, pel 2, blocks 8/4
FAULTING = geometry(36, 36, "gray", 8, 2, (0, 0), (8, 4))
SINGLE_BLOCK = geometry(16, 16, "420", 8, 1, (0, 0), (16, 0), levels=1)  # refused: the block is as large as the padded frame
NEARLY_SINGLE = [geometry(16, 16, "420", 8, 1, (2, 2), (16, 0), levels=1), geometry(18, 18, "420", 8, 1, (0, 0), (16, 0), levels=1), geometry(18, 18, "gray", 16, 2, (0, 0), (16, 0), levels=1)]

# geometries with an empty legal rectangle on some level, horizontally AND vertically (tests/test_search_addressing.py checks that they have)
EMPTY = [
    FAULTING,
    geometry(36, 36, "gray", 8, 2, (0, 0), (8, 4), shadow=False),
    geometry(36, 36, "gray", 16, 2, (0, 0), (8, 4)),
    geometry(36, 36, "gray", 16, 2, (0, 0), (8, 4), shadow=False),
    geometry(36, 36, "420", 8, 2, (0, 0), (8, 4)),
    geometry(36, 36, "420", 16, 2, (0, 0), (8, 4)),
    geometry(36, 36, "420", 16, 2, (0, 0), (8, 4), shadow=False),
]
# 72x40 without padding halves exactly twice (72, 36, 18 and 40, 20, 10: nothing is floored away) and 70x54 loses less than its grid does: their
# coarsest blocks stay inside their levels.  In the grid as unpadded clips whose rectangles are NOT empty
FULL_PAD0 = [
    geometry(72, 40, "420", 8, 2, (0, 0), (8, 4)),
    geometry(72, 40, "420", 16, 2, (0, 0), (8, 4)),
    geometry(70, 54, "420", 8, 2, (0, 0), (8, 4)),
]

# ordinary padded geometries of tests/test_gpu_parity.py: they must be clean, and were before the bias
ORDINARY = [
    geometry(128, 96, "420", 8, 2, (16, 16), (8, 4)),
    geometry(128, 96, "420", 16, 2, (16, 16), (8, 4)),
    geometry(640, 360, "420", 8, 1, (16, 16), (8, 0)),
    geometry(384, 224, "420", 16, 2, (16, 16), (16, 8)),
    geometry(512, 288, "420", 16, 2, (16, 16), (32, 16)),
    geometry(256, 144, "420", 8, 2, (16, 16), (16, 0)),
    geometry(256, 144, "420", 8, 2, (16, 16), (16, 8)),
    geometry(256, 144, "420", 8, 4, (16, 16), (8, 2)),
    geometry(130, 70, "420", 8, 2, (8, 8), (8, 4)),
]


def audit_grid():
    """every geometry the audit walks: the named ones, and 36x36 / 70x54 / 72x40 in Gray and 4:2:0 at 8 and 16 bits with every padding below
    the chroma ratio, pel 1 / 2 / 4, every block shape the lean and the specialised kernels admit, with and without the shadow planes"""
    out = list(EMPTY) + [SINGLE_BLOCK] + list(NEARLY_SINGLE) + list(FULL_PAD0) + list(ORDINARY)
    out.append(geometry(35, 30, "444", 8, 2, (0, 0), (8, 4)))  # 4:4:4: the generic kernel, 64-bit addresses
    for (w, h), fmt, bits, pad, pel, blk, shadow in itertools.product([(36, 36), (70, 54), (72, 40)], ("gray", "420"), (8, 16), PADS, (1, 2, 4), BLOCKS, (True, False)):
        if blk[0] == 32 and bits != 16:
            continue
        for extra in ([{}, dict(pelsearch=2)] if pel == 4 else [{}]):  # (pel 4 at pelsearch 4 is the general kernels'; at pelsearch 2 the lean kernels take it)
            g = geometry(w, h, fmt, bits, pel, pad, blk, shadow, **extra)
            if all(g["name"] != o["name"] for o in out):
                out.append(g)
    return out


def make(mod, g, num_frames=1 << 30, **akw):
    """(Super, Analyse) of `mod` -- the oracle or the product binding -- for a geometry; raises what the module raises for a refused one"""
    kw = dict(subsampling=SUB[g["fmt"]], gray=g["fmt"] == "gray", **g["skw"])
    if mod.__name__ == "mvtools_amd":
        kw["shadow"] = g["shadow"]
    sup = mod.Super(g["w"], g["h"], g["bits"], **kw)
    return sup, mod.Analyse(sup, num_frames, **dict(g["akw"], **akw))


def clip(g, n=5, seed=23, motion=(3, -2)):
    """n frames of a moving textured clip in the geometry's format (Gray: one plane)"""
    frames = pl.moving_clip(g["w"], g["h"], g["bits"], n, seed=seed, sub=SUB[g["fmt"]], noise=2, motion=motion)
    return [f[:1] for f in frames] if g["fmt"] == "gray" else frames


# ---- the GPU cases (tests/test_gpu_small_geometry.py; tests/test_small_geometry_cases.py shows on the oracle what they are good for)
GPU_SEARCHES = [
    FAULTING,
    geometry(36, 36, "gray", 16, 2, (0, 0), (8, 4)),
    geometry(36, 36, "gray", 16, 2, (0, 0), (8, 4), shadow=False),
    geometry(36, 36, "420", 8, 2, (0, 0), (8, 4)),
    geometry(36, 36, "420", 8, 2, (0, 0), (8, 4), shadow=False),
    geometry(36, 36, "420", 16, 2, (0, 0), (8, 4)),
    geometry(36, 36, "420", 16, 2, (0, 0), (8, 4), shadow=False),
    geometry(36, 36, "420", 8, 1, (0, 0), (8, 0)),
    geometry(36, 36, "420", 16, 4, (1, 1), (16, 8)),
    geometry(36, 36, "420", 8, 1, (2, 0), (16, 0)),
    geometry(72, 40, "420", 8, 2, (0, 0), (8, 4)),
    geometry(72, 40, "420", 16, 2, (0, 0), (16, 8)),
    geometry(72, 40, "420", 8, 2, (1, 1), (16, 8)),
    geometry(72, 40, "420", 16, 1, (0, 0), (16, 0)),
    geometry(70, 54, "420", 8, 2, (0, 0), (8, 4)),
    geometry(70, 54, "420", 16, 2, (1, 1), (32, 16)),
    geometry(70, 54, "420", 16, 4, (0, 0), (8, 0)),
    geometry(70, 54, "gray", 8, 2, (2, 0), (16, 8)),
    geometry(36, 36, "420", 16, 4, (0, 0), (8, 4), pelsearch=2),   # pel 4 in the lean and the speculative kernels (pelsearch 4 is the general kernels')
    geometry(36, 36, "420", 8, 4, (1, 1), (16, 8), pelsearch=2),
    geometry(35, 30, "444", 8, 2, (0, 0), (8, 4)),
    geometry(35, 30, "444", 16, 1, (1, 1), (8, 4)),
] + NEARLY_SINGLE  # (one block per frame; SINGLE_BLOCK itself is refused, tests/test_search_addressing.py)

# Analyse variations every GPU search case runs with: direction, distance (frame 4 of 5 with isb=1, delta 2 has its reference outside the clip), chroma, global
VARIANTS = [dict(isb=1, delta=1), dict(isb=0, delta=2), dict(isb=1, delta=2, chroma=0), dict(isb=0, delta=1, **{"global": 0})]


def routes(g, route):
    """the kernel routes a geometry can take, as (id, debug options, expected mvx_debug_last_launch [4]) -- route: out[23] of mvx_analyse_debug_level"""
    r = [("general", dict(general=1), 0), ("cpw1", dict(general=1, cpw1=1), 0)]
    if route == 2:
        r += [("spec0", dict(spec=0, team=0), 0), ("spec1", dict(spec=1), None), ("spec2", dict(spec=2, team=0), 2), ("spec3", dict(spec=3, team=0), 2), ("spec5", dict(spec=5, team=0), 2),
              ("team2", dict(spec=5, team=2), 3), ("team4", dict(spec=5, team=4), 3)]
    return r
