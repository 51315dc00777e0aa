"""What the AnalyseN / CompensateN tests share (test infrastructure): the cases, the jobs of a clip against a radius, and the share of
(block, field) pairs a CompensateN case compensates or falls back on.

The clip is the (1, 0)-per-frame moving texture of tests/degrain_n_cases.py at 96x64 with 2 * radius + 3 frames: every frame is a job, so the
first and the last radius frames have references outside the clip on one side.  With that motion the search still follows the texture at a
distance of 7, so most far blocks are compensated, and the rectangle that moves the other way leaves some that are not."""
import degrain_n_cases as dc
import vector_fields

W, H = 96, 64
B84 = ("p2", dict(pel=2), dict(blksize=8, overlap=4))     # overlapped blocks: 23 x 15 of them; cells of 4 luma / 2 chroma samples (4:4:4: 4 / 4)
B160 = ("p1", dict(pel=1), dict(blksize=16, overlap=0))   # blocks side by side: 6 x 4; cells of 16 / 8 samples (16 bits: 8 / 8)
B42 = ("p2b4", dict(pel=2), dict(blksize=4, overlap=2))   # the smallest blocks: 47 x 31 of them; at 4:2:0 chroma blocks of 2 stepping by 1 -- cells of ONE sample
RADII = (1, 2, 3, 7)

# fmt, bits, (tag, super kwargs, analyse kwargs)
GEOS = [("420", 8, B84), ("420", 8, B160), ("420", 16, B84), ("420", 16, B160), ("444", 8, B84), ("gray", 8, B160), ("420", 8, B42), ("420", 16, B42)]

# thsad of every CompensateN case: chosen on the CPU (tests/test_multi_cases.py) so that beyond distance 1 at least half of the (block, field)
# pairs are compensated and at least a fiftieth fall back on the source block (the shares it leaves: 0.64 .. 0.96 and 0.04 .. 0.36; the blocks of 4: 0.88 .. 0.96 and 0.04 .. 0.12)
THSAD = 250
USED, UNUSED = 0.5, 0.02


def cases():
    return [(fmt, bits, blk, radius) for fmt, bits, blk in GEOS for radius in RADII]


def case_id(c):
    fmt, bits, blk, radius = c
    return "%s-%dbit-blk%d-ov%d-%s-r%d" % (fmt, bits, blk[2]["blksize"], blk[2]["overlap"], blk[0], radius)


def nframes(radius):
    return 2 * radius + 3


def clip(fmt, bits, radius):
    return dc.clip(W, H, bits, nframes(radius), fmt)


def field_of(r):
    """field r -> (isb, delta)"""
    return int(r % 2 == 0), r // 2 + 1


def far_shares(sads, ad, th, radius):
    """sads[r]: the level-0 SADs of field r (every field valid) -> the shares of (block, field) pairs beyond distance 1 (radius 1: of all
    pairs) whose SAD is below / not below Compensate's scaled thsad"""
    scaled = vector_fields.scaled_thresholds(ad, th)[0]
    first = 2 if radius > 1 else 0
    below = sum(int((s < scaled).sum()) for s in sads[first:])
    total = sum(s.size for s in sads[first:])
    return below / total, 1 - below / total
