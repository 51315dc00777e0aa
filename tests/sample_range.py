"""Clips that reach the ENDS of the sample range, and the case lists built on them (no GPU, no oracle).

`pipeline.moving_clip` and `synth.survey_clip` are mid-grey: their samples never come near 0 or the depth's maximum pm, so neither the
`min(pm, max(0, v))` of the sub-pel filters nor the large block SADs of a fade or a cut were ever compared with anything.  Three
generators close that gap; each returns the same `frames[f][p]` layout as `moving_clip`:

  step(lo, hi)   frames alternate between two levels: block SADs close to blocksize * (hi - lo), up to the 2^27 bound of a 32x32
                 block at 16 bits -- the penalty products of the search (pnew * SAD) and the scene-change paths of the consumers
  rails          moving_clip's texture and motion with the contrast stretched about mid-range and hard-clipped: at least a tenth
                 of the samples exactly 0, a tenth exactly pm, real texture between -- clamps and limits at both ends on a clip the
                 search still follows
  checker        3x3 cells of 0 and pm moving by (2, 1) per frame: the bicubic and Wiener taps overshoot on both sides of every edge

The per-pixel Flow filters (FlowInter / FlowFPS, Flow, FlowBlur) have case lists of their own at the end of this file, on the same three
clips, with the vectors the search finds and with crafted fields (tests/vector_fields.py).

tests/test_sample_range.py proves through the oracle alone that each case reaches what it claims; tests/test_gpu_sample_range.py
runs the cases on the GPU.  tests/sample_range_oracle_main.c repeats `step` and `checker` in C (same arithmetic, same LCG).
"""
import numpy as np

import pipeline as pl
import vector_fields

DEPTHS = (8, 10, 12, 14, 16)


def _dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def _plane_dims(width, height, sub, p):
    return (width >> sub[0], height >> sub[1]) if p else (width, height)


def lcg_take(state, n):
    """n outputs of x <- x * 1664525 + 1013904223 (mod 2^32), bits 16..31 of each; returns (outputs, new state).  Sequential in
    uint64 numpy: the C program steps the same recurrence."""
    a, c = 1664525, 1013904223
    ak = np.cumprod(np.full(n, a, dtype=np.uint64))                      # a^1 .. a^n (mod 2^64; only the low 32 bits are used)
    with np.errstate(over="ignore"):
        s = np.cumsum(np.concatenate([[np.uint64(1)], ak[:-1]]))         # sum_{j<k} a^j
        st = (ak * np.uint64(state) + np.uint64(c) * s) & np.uint64(0xFFFFFFFF)
    return (st >> np.uint64(16)).astype(np.int64), int(st[-1])


def step(width, height, bits, nframes, lo, hi, sub=(1, 1), seed=12345):
    """Even frames lo + n, odd frames hi - n, n uniform in [0, range / 32] (pulled inwards: a level at an end of the range stays
    inside it), luma and chroma alike.  lo and hi are samples of the clip's own depth."""
    pm = (1 << bits) - 1
    assert 0 <= lo < hi <= pm
    amp = (1 << bits) // 32
    assert hi - lo > 2 * amp
    state = seed
    frames = []
    for f in range(nframes):
        planes = []
        for p in range(3):
            w, h = _plane_dims(width, height, sub, p)
            r, state = lcg_take(state, w * h)
            n = (r * (amp + 1)) >> 16                                    # 0 .. amp
            v = (hi - n) if (f & 1) else (lo + n)
            planes.append(v.reshape(h, w).astype(_dtype(bits)))
        frames.append(planes)
    return frames


def checker(width, height, bits, nframes, sub=(1, 1), cell=3):
    """cells of `cell` x `cell` samples of 0 and pm, in every plane's own grid, moving by (2, 1) samples per frame"""
    pm = (1 << bits) - 1
    frames = []
    for f in range(nframes):
        planes = []
        for p in range(3):
            w, h = _plane_dims(width, height, sub, p)
            x = np.arange(w)[None, :] - 2 * f + 3 * cell * nframes           # (offset: no negative operand, C and numpy divide alike)
            y = np.arange(h)[:, None] - f + 3 * cell * nframes
            planes.append((pm * ((x // cell + y // cell) & 1)).astype(_dtype(bits)))
        frames.append(planes)
    return frames


RAILS_GAIN = (4.0, 8.0, 8.0)  # luma texture spans about +-110 of 255 around 120, chroma +-20 around 128: both end up with a fifth or more of the samples on each rail


def rails(width, height, bits, nframes, sub=(1, 1), seed=7, noise=2, motion=(3, -1)):
    """moving_clip stretched about mid-range by RAILS_GAIN and hard-clipped to [0, pm]"""
    pm = (1 << bits) - 1
    mid = (pm + 1) // 2
    frames = []
    for fr in pl.moving_clip(width, height, bits, nframes, seed=seed, noise=noise, motion=motion, sub=sub):
        planes = []
        for p, plane in enumerate(fr):
            v = mid + np.rint((plane.astype(np.float64) - mid) * RAILS_GAIN[p])
            planes.append(np.clip(v, 0, pm).astype(_dtype(bits)))
        frames.append(planes)
    return frames


def make(gen, width, height, bits, nframes, sub=(1, 1), **kw):
    """a clip by generator name; "step" needs lo= and hi="""
    if gen == "step":
        return step(width, height, bits, nframes, kw.pop("lo"), kw.pop("hi"), sub=sub, **kw)
    return {"rails": rails, "checker": checker}[gen](width, height, bits, nframes, sub=sub, **kw)


def widen(frames):
    """the same samples as a 16-bit clip (a 16-bit Super of them clamps at 65535 only: what the real depth's clamp cut off shows)"""
    return [[p.astype(np.uint16) for p in f] for f in frames]


def zero_vector_luma_sad(frames, blk, overlap):
    """level-0 luma SAD of every block against the same position of the next frame: int64 array (nBlkY, nBlkX), MVAnalyse.c:412-420 geometry"""
    a, b = frames[0][0].astype(np.int64), frames[1][0].astype(np.int64)
    h, w = a.shape
    stepxy = blk - overlap
    nbx, nby = (w - overlap) // stepxy, (h - overlap) // stepxy
    d = np.abs(a - b)
    return np.array([[d[by * stepxy: by * stepxy + blk, bx * stepxy: bx * stepxy + blk].sum() for bx in range(nbx)] for by in range(nby)])


# ---------------------------------------------------------------------------------------------------------------- Super
# (gen, w, h, bits, sub, super kwargs).  136x72: the smallest frame of the existing pel-4 cases; 138 / 150 wide: the rows-in-registers
# level-0 kernel's ragged widths, hpad 5 sends the same clip through the tile kernel instead.
def _super_cases():
    out = []
    for gen in ("checker", "rails"):
        for bits in (10, 12, 14, 16):
            for sharp in (1, 2):
                for pel in (2, 4):
                    out.append((gen, 136, 72, bits, (1, 1), dict(sharp=sharp, pel=pel)))
            out.append((gen, 136, 72, bits, (1, 1), dict(sharp=0)))
        for sharp in (0, 1, 2):
            out.append((gen, 136, 72, 8, (1, 1), dict(sharp=sharp)))
        out.append((gen, 134, 78, 10, (0, 0), dict(hpad=4, vpad=4)))
        out.append((gen, 160, 96, 10, (1, 0), {}))
        for bits in (10, 14):
            out.append((gen, 138, 70, bits, (1, 1), {}))                           # rows-in-registers kernel
            out.append((gen, 150, 90, bits, (1, 1), dict(hpad=5, vpad=3)))         # alignment rule fails: tile kernel
            out.append((gen, 150, 66, bits, (1, 1), dict(sharp=1, hpad=2, vpad=2)))
    for rf in range(5):
        out.append(("checker", 144, 80, 12, (1, 1), dict(rfilter=rf)))
    return out


SUPER_CASES = _super_cases()


def super_overshoot_cases():
    """the cases whose taps must overshoot: sharp 1 or 2 (an absent sharp is 2) at 10, 12 and 14 bits, sub-pel planes present"""
    return [c for c in SUPER_CASES if c[3] in (10, 12, 14) and c[5].get("sharp", 2) in (1, 2) and c[5].get("pel", 2) > 1]


# -------------------------------------------------------------------------------------------------------------- Analyse
# (name, bits, sub, lo, hi, analyse kwargs); all 256x160.
# "penalty": pnew * (zero-vector luma SAD) >= 2^31 on at least half of the blocks -- where a 32-bit product wraps.
PENALTY_CASES = [
    ("fade-to-69%", 16, (1, 1), 0, 45000, dict(blksize=32, overlap=16)),          # the benchmark's cfg5 shape, default pnew (50)
    ("fade-to-white", 16, (1, 1), 20000, 65535, dict(blksize=32, overlap=16)),
    ("b16-pnew256", 16, (1, 1), 0, 39000, dict(blksize=16, overlap=8, pnew=256)),
    ("b32-pnew256", 16, (1, 1), 0, 65535, dict(blksize=32, overlap=16, pnew=256)),
]
# 4:4:4, 16x16, pnew 256: the chroma SAD (U + V = twice the luma SAD) passes 2^31 / 256 while the luma SAD stays below it:
# 256 samples * (26000 - about 2 * 1024 of noise) = 6.1e6 < 8 388 608 <= 12.3e6
PENALTY_444_CASE = ("444-chroma-only", 16, (0, 0), 0, 26000, dict(blksize=16, overlap=8, pnew=256))
# controls: cannot wrap.  0 -> 65535 at the default pnew: 50 * 2^26 = 3.4e9 DOES pass 2^31 but every candidate's SAD is the same here, so
# the winner does not depend on the penalty; it pins the bound of the SUM (block SAD < 2^27).  8 and 14 bits: 256 * (16 * 16 * 16383) =
# 1.07e9 < 2^31, chroma (2 * 8 * 8 * 16383) smaller still -- no depth below 16 can reach the product's bound with blocks up to 16x16.
CONTROL_CASES = [
    ("full-swing-defaults", 16, (1, 1), 0, 65535, dict(blksize=32, overlap=16)),
    ("8bit-pnew256", 8, (1, 1), 0, 255, dict(blksize=16, overlap=8, pnew=256)),
    ("14bit-pnew256", 14, (1, 1), 0, 16383, dict(blksize=16, overlap=8, pnew=256)),
]
STEP_W, STEP_H = 256, 160

# rails through the search: (name, bits, analyse kwargs) on RAILS_W x RAILS_H, which holds 3x3 blocks of 16 at the coarsest level the search uses
RAILS_ANALYSE_CASES = [
    ("rails10", 10, dict(blksize=16, overlap=8)),
    ("rails12", 12, dict(blksize=16, overlap=8)),
    ("rails14", 14, dict(blksize=16, overlap=8)),
    ("rails16", 16, dict(blksize=16, overlap=8)),
    ("rails16-dct5", 16, dict(blksize=16, overlap=8, dct=5)),
    ("rails16-dct9", 16, dict(blksize=8, overlap=4, dct=9)),
    ("rails16-rescue", 16, dict(blksize=16, overlap=8, badsad=300, badrange=8)),
]
RAILS_W, RAILS_H = 192, 112

# ------------------------------------------------------------------------------------------------ Degrain / Compensate / BlockFPS
# (gen, w, h, bits, radius, analyse kwargs, degrain kwargs); limit: about 1 % of the range.  196 wide: no multiple of the cell -> the
# per-sample kernel takes the ragged cells beside the vectorised gather.
def _limit(bits):
    return max(1, ((1 << bits) - 1) // 100)


# checker: 3x3 cells moving by (2, 1) alias -- the search cannot follow them, every block SAD is above the default thscd1 and Degrain would
# only copy its source (the step cases cover that).  With thscd1 / thscd2 at their maxima and thsad close to its own every reference stays
# in the blend: weights and limits act on samples that are all 0 or pm.
CHECKER_BLEND = dict(thscd1=16320, thscd2=255, thsad=16000, thsadc=16000)


def _degrain_cases():
    out = []
    for gen in ("rails", "checker"):
        for bits in (10, 12, 14, 16):
            lim = dict(limit=_limit(bits), limitc=_limit(bits))
            if gen == "checker":
                out.append((gen, 128, 96, bits, 1, dict(blksize=8, overlap=4), dict(lim, **CHECKER_BLEND)))
                out.append((gen, 128, 96, bits, 1, dict(blksize=16, overlap=0), dict(CHECKER_BLEND)))
                out.append((gen, 196, 116, bits, 3, dict(blksize=16, overlap=8), dict(lim if bits in (10, 16) else {}, **CHECKER_BLEND)))
                out.append((gen, 128, 96, bits, 3, dict(blksize=16, overlap=0), dict({} if bits in (10, 16) else lim, **CHECKER_BLEND)))
                continue
            out.append((gen, 128, 96, bits, 1, dict(blksize=8, overlap=4), lim))
            out.append((gen, 128, 96, bits, 1, dict(blksize=16, overlap=0), {}))
            out.append((gen, 196, 116, bits, 3, dict(blksize=16, overlap=8), lim if bits in (10, 16) else {}))
            out.append((gen, 128, 96, bits, 3, dict(blksize=16, overlap=0), {} if bits in (10, 16) else lim))
    for bits in (10, 16):
        out.append(("step", 128, 96, bits, 1, dict(blksize=8, overlap=4), {}))     # every reference is a scene change away
        out.append(("step", 128, 96, bits, 1, dict(blksize=16, overlap=0), dict(limit=_limit(bits), limitc=_limit(bits))))
    return out


DEGRAIN_CASES = _degrain_cases()
STEP_SPAN = {8: (0, 255), 10: (0, 1023), 12: (0, 4095), 14: (0, 16383), 16: (0, 65535)}  # the step clip of the consumers: end to end

# (gen, w, h, bits, analyse kwargs, compensate kwargs)
COMPENSATE_CASES = [(gen, 128, 96, bits, dict(blksize=8, overlap=4) if bits == 10 else dict(blksize=16, overlap=8), ckw)
                    for gen in ("rails", "step") for bits in (10, 16)
                    for ckw in ({}, dict(thsad=1), dict(scbehavior=0), dict(thsad=1, scbehavior=0))]

# (gen, w, h, bits, analyse kwargs, blockfps kwargs)
BLOCKFPS_CASES = [("rails", 128, 96, (10, 16)[m & 1], dict(blksize=8, overlap=4), dict(num=60, den=1, mode=m, ml=40.0)) for m in range(6)] + [
    ("step", 128, 96, 16, dict(blksize=8, overlap=4), dict(num=60, den=1)),
    ("step", 128, 96, 16, dict(blksize=8, overlap=4), dict(num=60, den=1, blend=0)),
]

# ---------------------------------------------------------------------------------------- FlowInter / FlowFPS, Flow, FlowBlur
# (gen, fmt, w, h, bits, super kwargs, analyse kwargs, filter kwargs, recipe or None, kinds): the case shape of tests/test_gpu_flow.py and
# tests/test_gpu_flowmc.py with the clip's generator in front, a vector_fields.Recipe where the vectors are crafted (None: the vectors the
# search finds) and at the end what the restatement reports the output frames took.  Every case runs FLOW_NF input frames.
#
# Searched vectors on rails or checker never reach a formula at the default thresholds: the block SADs of a clip with a fifth of its samples
# on each rail are above thscd1 = 400 in more than thscd2 = 130 of 256 blocks, the blobs count as scene changes and every job is Blend.  T
# (both thresholds at their maxima) keeps them usable; the crafted fields carry SADs of 64 at most and need no T.
FLOW_NF = 4
FLOW_FORMATS = {"420": (1, 1), "444": (0, 0), "422": (1, 0), "gray": (1, 1)}
T = dict(thscd1=16320, thscd2=255)
_B84 = dict(blksize=8, overlap=4)
_BW, _FW = dict(_B84, isb=1), dict(_B84, isb=0)


def flow_clip(gen, fmt, w, h, bits, nframes=FLOW_NF):
    """the clip of a Flow case: rails with moving_clip's noise of the Flow suites (3), step from end to end of the range (STEP_SPAN), checker;
    luma only for gray"""
    sub = FLOW_FORMATS[fmt]
    if gen == "rails":
        frames = rails(w, h, bits, nframes, sub=sub, noise=3)
    elif gen == "step":
        frames = step(w, h, bits, nframes, *STEP_SPAN[bits], sub=sub)
    else:
        frames = make(gen, w, h, bits, nframes, sub=sub)
    return [[f[0]] for f in frames] if fmt == "gray" else frames


def _flowinter_range_cases():
    R = vector_fields.Recipe
    out = []
    for bits in (10, 12, 14, 16):          # searched vectors, T: the formulas on samples of 0 and pm with the masks the search's vectors give
        for fkw, kinds in ((dict(fps=1, num=60, mask=2), "copy,extra,simple"), (dict(fps=1, num=48, mask=2), "copy,extra128,simple128"),
                           (dict(fps=1, num=48, mask=0), "copy,simple128"), (dict(fps=1, num=60, mask=1), "copy,regular"),
                           (dict(time=50.0), "blend,extra128,regular128"), (dict(time=33.0, ml=20.0), "blend,extra,regular")):
            out.append(("rails", "420", 128, 96, bits, {}, _B84, dict(fkw, **T), None, kinds))
    out += [
        ("rails", "444", 128, 96, 10, {}, _B84, dict(fps=1, num=60, mask=2, **T), None, "copy,extra,simple"),
        ("rails", "422", 160, 96, 12, {}, _B84, dict(time=50.0, **T), None, "blend,extra128,regular128"),
        ("rails", "gray", 128, 96, 14, {}, _B84, dict(fps=1, num=48, mask=2, **T), None, "copy,extra128,simple128"),
        ("rails", "420", 206, 118, 10, {}, _B84, dict(fps=1, num=60, mask=1, **T), None, "copy,regular"),     # nBlkXP > nBlkX and nBlkYP > nBlkY
    ]
    seed = 2000                            # crafted occlusion fields: saturated masks; at 16 bits the regular formula's 32-bit product on its bound
    for fkw, kinds in ((dict(fps=1, num=48, mask=1), "copy,regular128"), (dict(fps=1, num=60, mask=1), "copy,regular")):
        for gen in ("rails", "checker", "step"):
            out.append((gen, "420", 128, 96, 16, {}, _B84, fkw, R("occlusion", seed), kinds))
            seed += 20
    for bits in (10, 12, 14):              # 255-masks on samples that are all 0 or pm, through Extra and Simple
        out.append(("checker", "420", 128, 96, bits, {}, _B84, dict(fps=1, num=60, mask=2), R("occlusion", seed), "copy,extra,simple"))
        out.append(("checker", "420", 128, 96, bits, {}, _B84, dict(fps=1, num=48, mask=0), R("occlusion", seed + 20), "copy,simple128"))
        seed += 40
    for bits in (10, 16):                  # the cut: Blend and the left frame between a frame near 0 and a frame near pm, default thresholds
        out += [
            ("step", "420", 128, 96, bits, {}, _B84, dict(fps=1, num=60, mask=2), None, "blend,copy"),
            ("step", "420", 128, 96, bits, {}, _B84, dict(fps=1, num=60, mask=2, blend=0), None, "copy,left"),
            ("step", "420", 128, 96, bits, {}, _B84, dict(time=33.0), None, "blend"),
            ("step", "420", 128, 96, bits, {}, _B84, dict(time=33.0, blend=0), None, "left"),
        ]
    return out


def _flow_range_cases():
    R = vector_fields.Recipe
    SH, FE = "collide,copy,hole,shift", "copy,fetch"
    out, seed = [], 2300
    for gen, bits in (("rails", 10), ("rails", 12), ("rails", 14), ("checker", 10)):   # crafted limits fields: the hole value of every depth
        for akw, fkw, kinds in ((_BW, dict(time=100.0, mode=1), SH), (_FW, dict(time=100.0, mode=1), SH), (_BW, dict(time=37.5, mode=1), SH),
                                (_FW, dict(time=37.5, mode=1), SH), (_BW, dict(time=100.0), FE)):
            out.append((gen, "420", 128, 96, bits, {}, akw, fkw, R("limits", seed), kinds))
            seed += 20
    out += [
        ("rails", "420", 128, 96, 16, {}, _BW, dict(time=100.0, mode=1), R("limits", seed), SH),
        ("rails", "420", 128, 96, 16, {}, _FW, dict(time=100.0), R("limits", seed + 20), FE),
        ("rails", "gray", 128, 96, 12, {}, _FW, dict(time=100.0, mode=1), R("limits", seed + 40), SH),
        ("rails", "420", 128, 96, 10, {}, _BW, dict(time=100.0, mode=1, **T), None, SH),                       # the vectors the search finds
        ("rails", "420", 128, 96, 14, {}, _FW, dict(time=100.0, mode=1, **T), None, SH),
    ]
    return out


def _blur_range_cases():
    R = vector_fields.Recipe
    K = "blur,copy,taps,trunc"
    out = [("rails", "420", 128, 96, bits, {}, _B84, dict(blur=200.0), R("limits", 2800 + 20 * i), K) for i, bits in enumerate((10, 12, 14, 16))]
    out += [
        ("rails", "420", 128, 96, 12, {}, _B84, dict(blur=200.0, prec=3), R("limits", 2880), "blur,copy,notaps,taps,trunc"),
        ("step", "420", 128, 96, 16, {}, _B84, dict(blur=200.0), R("limits", 2900), K),                           # the largest tap sums there are
        ("checker", "420", 128, 96, 16, {}, _B84, dict(blur=200.0), R("limits", 2920), K),
        ("checker", "420", 128, 96, 10, {}, _B84, dict(blur=200.0), R("limits", 2940), K),
    ]
    return out


FLOWINTER_RANGE_CASES = _flowinter_range_cases()
FLOW_RANGE_CASES = _flow_range_cases()
BLUR_RANGE_CASES = _blur_range_cases()


def flow_case_id(c):
    kw = ",".join("%s=%s" % kv for kv in c[7].items() if kv[0] not in T) + (",T" if "thscd1" in c[7] else "")
    return "%s-%s-%dx%d-%dbit-%s%s-%s" % (c[0], c[1], c[2], c[3], c[4], "isb%d-" % c[6]["isb"] if "isb" in c[6] else "", kw, c[8] if c[8] is not None else "searched")
