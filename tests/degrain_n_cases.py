"""What the DegrainN tests share (test infrastructure): clips whose motion the search still follows at a temporal distance of 24, the
job of one output frame at a radius, and the restatement (tests/degrain_n_ref.py) set up from a filter's resolved thresholds.

On the suite's moving_clip with its default motion (3, -1) the search loses the motion beyond distance 5, every far weight is 0, and a DegrainN
that ignored the far references would pass.  With motion (1, 0) most far (block, reference) pairs keep a weight and some do not."""
import pipeline as pl
import vector_fields

import degrain_n_ref

FORMATS = {"420": {}, "444": dict(subsampling=(0, 0)), "422": dict(subsampling=(1, 0)), "gray": dict(gray=True)}


def clip(w, h, bits, n, fmt="420", seed=31, noise=3):
    f = FORMATS[fmt]
    frames = pl.moving_clip(w, h, bits, n, seed=seed, noise=noise, motion=(1, 0), sub=f.get("subsampling", (1, 1)))
    return [[fr[0]] for fr in frames] if f.get("gray") else frames


def neighbours(target, radius, nframes):
    """[(reference index r, isb, delta, frame number or None when it lies outside the clip)] in the order mvbw, mvfw, mvbw2, mvfw2, ..."""
    out = []
    for d in range(1, radius + 1):
        for isb in (1, 0):
            nref = target + (d if isb else -d)
            out.append((len(out), isb, d, nref if 0 <= nref < nframes else None))
    return out


def restatement(oracle, radius, ad, th_luma, th_chroma, dkw, gray=False):
    """tests/degrain_n_ref.py for a filter whose scaled thresholds per distance are th_luma / th_chroma; dkw: the filter's other arguments"""
    _, s1, s2 = vector_fields.scaled_thresholds(ad, 400, dkw.get("thscd1", 400), dkw.get("thscd2", 130))
    return degrain_n_ref.DegrainN(oracle, radius, ad, th_luma, th_chroma, s1, s2, plane=dkw.get("plane", 4), limit=dkw.get("limit"),
                                  limitc=dkw.get("limitc"), gray=gray)


B84, B168 = dict(blksize=8, overlap=4), dict(blksize=16, overlap=8)
A = ("420", 128, 96, 8, {}, B84)       # four-sample luma cells, two-sample chroma cells
B = ("420", 204, 116, 16, {}, B168)    # eight / four; a 4-sample strip right and below that no block covers
B24 = ("420", 332, 196, 16, {}, B168)  # the same at radius 24: on B the search (blocks of 16, a small pyramid) loses a motion of 15 samples and more, and no reference
                                       # beyond distance 14 is usable
FAR24 = dict(thsad=1200)               # at radius 24 the default 400 keeps too few of the far references


def _large_cases():
    out = []
    for radius in (7, 8, 9, 12, 24):   # 14, 16, 18, 24 and 48 references: lists on both sides of every multiple of the gather's chunk of four
        for geo in (A, B24 if radius == 24 else B):
            out.append(geo + (radius, dict(FAR24) if radius == 24 else {}))
    out += [
        ("420", 160, 96, 8, {}, dict(blksize=8, overlap=0), 8, {}),                          # blocks side by side
        ("420", 256, 160, 8, {}, dict(blksize=32, overlap=16), 8, {}),
        ("420", 128, 96, 8, {}, dict(blksize=8, blksizev=4, overlap=4, overlapv=2), 8, {}),  # 8x4
        ("420", 128, 96, 8, {}, dict(blksize=4, overlap=2), 8, {}),                          # 4/2: chroma blocks of 2 stepping by 1 -- one-sample cells
        ("420", 128, 96, 8, dict(pel=1), B84, 8, {}),
        ("420", 128, 96, 16, dict(pel=4), B84, 8, {}),
        ("420", 144, 80, 10, {}, dict(blksize=16, overlap=4), 7, {}),                        # 10 bits; steps of 12 (chroma 6): cells of 4 and 2
        ("444", 128, 96, 8, {}, B84, 9, {}),
        ("422", 160, 96, 16, {}, B168, 7, {}),
        ("gray", 128, 96, 8, {}, B84, 12, {}),
    ]
    out += [A + (8, dict(plane=p)) for p in range(5)]
    # thsad2 = thsad / 4 (with thsad 400 no reference beyond distance 6 would keep a weight at radius 8)
    out += [A + (8, dict(limit=1, limitc=0)), A + (8, dict(thsad=1600, thsad2=400)), A + (24, dict(thsad=1200, thsad2=300, thsadc=1000, thsadc2=250))]
    return out


# fmt, w, h, bits, super kwargs, analyse kwargs, radius, DegrainN kwargs: each is run on the middle frame of 2 * radius + 1 against the restatement
LARGE_CASES = _large_cases()


def case_id(c):
    fmt, w, h, bits, skw, akw, radius, dkw = c
    kws = ",".join("%s=%s" % kv for d in (skw, akw, dkw) for kv in sorted(d.items()))
    return "%s-%dx%d-%dbit-r%d-%s" % (fmt, w, h, bits, radius, kws)


def threshold(t1, t2, radius, d):
    """the threshold at distance d before scaling (include/mvtools_amd.h, mv.DegrainN)"""
    import math
    if radius == 1 or t1 == t2:
        return t1
    return int(math.floor(t2 + (t1 - t2) * (1 + math.cos(math.pi * (d - 1) / (radius - 1))) / 2 + 0.5))


def tables(ad, radius, dkw):
    """the scaled thresholds per distance (luma, chroma) of a DegrainN with the arguments dkw, from the formula in Python doubles"""
    t1 = dkw.get("thsad", 400)
    t1c = dkw.get("thsadc", t1)
    t2, t2c = dkw.get("thsad2", t1), dkw.get("thsadc2", t1c)
    old = dkw.get("thscd1", 400)
    norm = lambda t: vector_fields.scaled_thresholds(ad, t, old)[0]
    return [norm(threshold(t1, t2, radius, d)) for d in range(1, radius + 1)], [norm(threshold(t1c, t2c, radius, d)) for d in range(1, radius + 1)]


FAR_USED, FAR_UNUSED = 0.5, 0.02   # every LARGE case: at least these shares of its (block, reference) pairs beyond distance 6 have W > 0 / W == 0


def far_shares_ok(ref):
    used, unused = ref.shares(7)
    return used >= FAR_USED and unused >= FAR_UNUSED, "beyond distance 6: %.3f of the weights > 0, %.3f == 0" % (used, unused)


# the ends of the sample range at radius 8, 16 bits (tests/sample_range.py): `step` alternates between 0 and 65535 -- every odd distance is a scene change
# away, every even one is the same level again, so half of the far pairs carry a weight and half none; `rails` is the moving clip stretched until a fifth
# of its samples sit on each rail.  Products stay below 2^31: 256 x 65535 + 128.
RANGE_GEO = ("420", 128, 96, 16, {}, B84)
RANGE_GENS = ("step", "rails")


def range_clip(gen, n):
    import sample_range as sr
    _, w, h, bits, _, _ = RANGE_GEO
    return sr.step(w, h, bits, n, 0, 65535) if gen == "step" else sr.rails(w, h, bits, n, motion=(1, 0))
