"""Crafted level-0 vector fields for the filters that consume MVTools_vectors blobs (test infrastructure, plain numpy).

Analyse on the suite's synthetic clips gives nearly constant fields: short vectors, no block on a limit of its search rectangle, neighbouring
vectors two sub-pel steps apart at most, no SAD on a threshold.  The editors here take a complete blob from Analyse (header, sizes and the
coarser levels stay) and rewrite level 0 so that a consumer meets what is legal but rare:

  limits       every block on, or uniformly inside, its legal rectangle (GroupOfPlanes / PlaneOfBlocks: oracle/mvo_analyse.c:580-583)
  sad_edges    SADs on and around a threshold, 0, and one with the high dword set
  scene_count  exactly k blocks above thscd1 (the usable test is `count > thscd2`), the k blocks last in the blob
  occlusion    piecewise-constant fields whose steps give occlusion spans of several blocks, spans cut at the grid's ends, saturated and
               unsaturated mask values (MaskFun.cpp:86-130 MakeVectorOcclusionMaskTime)
  invalid      the validity word cleared

tests/test_vector_fields.py checks on the CPU that each field is what it claims for every case listed at the end of this file;
tests/test_gpu_vector_fields.py runs the same cases through the HIP consumers against the oracle / the restatements.
"""
import ctypes as C

import numpy as np

SAD_HIGH = 2 ** 33 + 5   # a SAD whose high dword is set (the blob stores int64)


# ------------------------------------------------------------------ blob access

def level_span(blob, ad, level=0):
    """(byte offset of the first record, block rows, block columns) of one level of a blob.  Fakery.c:110-121: after the two header ints
    the planes follow coarsest first, each led by its own size in bytes; the grid of level i is the reference's (GroupOfPlanes.c:38-47)."""
    b = np.asarray(blob, dtype=np.uint8)
    nwb = (ad.nBlkSizeX - ad.nOverlapX) * ad.nBlkX + ad.nOverlapX
    nhb = (ad.nBlkSizeY - ad.nOverlapY) * ad.nBlkY + ad.nOverlapY
    off = 8
    for i in range(ad.nLvCount - 1, -1, -1):
        bx = ((nwb >> i) - ad.nOverlapX) // (ad.nBlkSizeX - ad.nOverlapX)
        by = ((nhb >> i) - ad.nOverlapY) // (ad.nBlkSizeY - ad.nOverlapY)
        if i == level:
            assert off + 4 + bx * by * 16 <= b.size, "blob too short for its analysis data"
            return off + 4, by, bx
        off += int(b[off:off + 4].view(np.int32)[0])
    raise ValueError(level)


def records(blob, ad, level=0):
    """writable views (xy: int32 (rows, columns, 4) of which [..., 0] = x and [..., 1] = y; sad: int64 (rows, columns)) into a uint8 blob"""
    off, by, bx = level_span(blob, ad, level)
    rec = blob[off:off + by * bx * 16]
    return rec.view(np.int32).reshape(by, bx, 4), rec.view(np.int64).reshape(by, bx, 2)[:, :, 1]


def _fresh(blob):
    return np.array(blob, dtype=np.uint8, copy=True)


# ------------------------------------------------------------------ geometry and thresholds

def legal_rect(ad, margin=0):
    """per block column (xmin, xmax) and per block row (ymin, ymax), inclusive, in sub-pel units: level 0 of oracle/mvo_analyse.c:580-583
    (PlaneOfBlocks.cpp: nDxMin .. nDxMax - 1).  margin shrinks the rectangle on every side."""
    def axis(n, blk, ov, size, pad):
        pos = np.arange(n, dtype=np.int64) * (blk - ov)
        return -(pos + pad) * ad.nPel + margin, (size + pad - pos - blk) * ad.nPel - 1 - margin
    xmin, xmax = axis(ad.nBlkX, ad.nBlkSizeX, ad.nOverlapX, ad.nWidth, ad.nHPadding)
    ymin, ymax = axis(ad.nBlkY, ad.nBlkSizeY, ad.nOverlapY, ad.nHeight, ad.nVPadding)
    return xmin, xmax, ymin, ymax


def scaled_thresholds(ad, thsad, thscd1=400, thscd2=130):
    """(thSAD, nSCD1, nSCD2) as Degrain and Compensate scale them: MVAnalysisData.c:7-31 scaleThSCD through the oracle, then
    thSAD = thsad * nSCD1 / thscd1 (MVDegrains.cpp:658-659, MVCompensate.c:521)"""
    import mvoracle
    L = mvoracle.lib()
    a = mvoracle.AnalysisData.from_buffer_copy(bytes(ad))
    s1, s2 = C.c_int64(thscd1), C.c_int(thscd2)
    L.mvo_scale_thscd.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(mvoracle.AnalysisData)]
    L.mvo_scale_thscd(C.byref(s1), C.byref(s2), C.byref(a))
    return thsad * s1.value // thscd1, s1.value, s2.value


def degrain_weight(th, sad):
    """MVDegrains.h:184-189 DegrainWeight"""
    th, sad = int(th), int(sad)
    if sad >= th:
        return 0
    return int((th - sad) * (th + sad) * 256 / float(th * th + sad * sad))


def normalised_weights(wrefs):
    """MVDegrains.h:208-223: (WSrc, WRefs) after normalising to a sum of 256"""
    s = 256 + sum(wrefs)
    out = [w * 256 // s for w in wrefs]
    return 256 - sum(out), out


def recalculate_threshold(rc):
    """Recalculate's scaled thSAD (MVRecalculate.c, through the oracle's structure rc.d), brought to the old clip's block area: the old SAD
    is scaled by new area / old area before it becomes the predictor's (PlaneOfBlocks.cpp:1321)"""
    new, old = rc.d.an.ad, rc.d.old
    return int(rc.d.thSAD) * (old.nBlkSizeX * old.nBlkSizeY) // (new.nBlkSizeX * new.nBlkSizeY)


def flowinter_time256(fkw):
    """the time256 an occlusion field is sized for: FlowInter's own (MVFlowInter.c:485, float arithmetic), 128 for FlowFPS"""
    return 128 if fkw.get("fps") else int(np.float32(fkw.get("time", 50.0)) * np.float32(256.0) / np.float32(100.0))


# ------------------------------------------------------------------ the recipes: each returns an edited copy of the blob

def limits(blob, ad, seed, margin=0, sad_max=64):
    """each component independently: a quarter of the blocks on the minimum, a quarter on the maximum, the rest uniform in between;
    SADs small (0 .. sad_max), so every block is used with a weight"""
    b = _fresh(blob)
    rng = np.random.default_rng(seed)
    xy, sad = records(b, ad)
    by, bx = sad.shape
    xmin, xmax, ymin, ymax = legal_rect(ad, margin)
    for comp, lo, hi in ((0, np.broadcast_to(xmin[None, :], (by, bx)), np.broadcast_to(xmax[None, :], (by, bx))),
                         (1, np.broadcast_to(ymin[:, None], (by, bx)), np.broadcast_to(ymax[:, None], (by, bx)))):
        pick = rng.integers(0, 4, (by, bx))
        xy[:, :, comp] = np.where(pick == 0, lo, np.where(pick == 1, hi, rng.integers(lo, hi + 1)))
    sad[:, :] = rng.integers(0, sad_max + 1, (by, bx))
    return b


def sad_mask_values(sad, ad, ml):
    """the value 255 * sad * factor of MaskFun.cpp:133-166 MakeSADMaskTime before it is cut at 255 (gamma 1), per block, with BlockFPS's
    factor 4 / (ml * nBlkSizeX * nBlkSizeY) (MVBlockFPS.c) and the SAD brought to the 8-bit scale"""
    return 255.0 * (np.asarray(sad, np.int64) >> (ad.bitsPerSample - 8)) * (4.0 / (ml * ad.nBlkSizeX * ad.nBlkSizeY))


def sad_edge_values(th):
    return [0, 1, th // 2, th - 1, th, th + 1, 3 * th, SAD_HIGH]


def sad_edges(blob, ad, seed, th):
    """the vectors stay; every SAD is one of the eight values around the threshold th, drawn uniformly"""
    b = _fresh(blob)
    rng = np.random.default_rng(seed)
    _, sad = records(b, ad)
    sad[:, :] = np.array(sad_edge_values(th), np.int64)[rng.integers(0, 8, sad.shape)]
    return b


def scene_count(blob, ad, seed, thscd1, k, thsad):
    """the vectors stay; the last k blocks of the blob get thscd1 + 1, a tenth of the others exactly thscd1 (not counted), the rest less
    than thsad / 4 (and than thscd1)"""
    b = _fresh(blob)
    rng = np.random.default_rng(seed)
    _, sad = records(b, ad)
    flat = rng.integers(0, max(min(thsad // 4, thscd1), 1), sad.size)
    flat[rng.random(sad.size) < 0.1] = thscd1
    assert 0 <= k <= sad.size
    if k:
        flat[-k:] = thscd1 + 1
    sad[:, :] = flat.reshape(sad.shape)
    return b


def invalid(blob, ad, seed=0):
    b = _fresh(blob)
    b[4:8].view(np.int32)[0] = 0
    return b


def occlusion_terms(ad, mask_time, ml):
    """(time4096X, time4096Y, occnormX, occnormY) of MaskFun.cpp:94-97"""
    sx, sy = ad.nBlkSizeX - ad.nOverlapX, ad.nBlkSizeY - ad.nOverlapY
    return mask_time * 16 // (sx * ad.nPel), mask_time * 16 // (sy * ad.nPel), 80.0 / (ml * sx * ad.nPel), 80.0 / (ml * sy * ad.nPel)


def _profile(n, lo, hi, t4096, norm, rng, last_big=True):
    """one line of n vector components (legal range lo[i] .. hi[i]) that is 0 except for falling steps between disjoint neighbour pairs:
    a step that spans three extra blocks at the first pair, at the last pair (last_big; else an unsaturated step there, the only kind
    that reaches the last block in a forward mask) and at every third pair in between, the smallest saturated step and an unsaturated step
    at the others"""
    big = -(-4096 * 3 // t4096)                                   # smallest o with o * t4096 / 4096 >= 3
    big = max(big, int(np.ceil(1.0 / norm)) + 1)                  # ... and a saturated value
    mid = max(1, int(0.5 / norm))                                 # a value near 127
    sat = int(np.ceil(1.0 / norm))                                # the smallest saturated step: a short span, so a forward range keeps it
    assert 1 <= int(255 * mid * norm) <= 254, "no unsaturated step exists at this ml"
    line = np.zeros(n, np.int64)
    pairs = [0, n - 2] + [int(c) for c in range(3, n - 4, 3)]
    for j, c in enumerate(pairs):
        if j == 0 or (j == 1 and last_big) or (j > 1 and j % 3 == 2):
            o = big
        elif j > 1 and j % 3 == 0:
            o = sat
        else:
            o = mid + int(rng.integers(0, 2)) * (mid > 1)
        a_lo, a_hi = lo[c + 1] + o, hi[c]
        assert a_lo <= a_hi, "a step of %d does not fit the legal rectangles of blocks %d and %d" % (o, c, c + 1)
        a = int(min(max(o // 2, a_lo, lo[c]), a_hi))
        line[c], line[c + 1] = a, a - o
    assert np.all(line >= lo) and np.all(line <= hi)
    return line


def occlusion(blob, ad, seed, time256, ml=100.0, sad_max=64):
    """piecewise-constant field: vx follows a column profile (two variants, alternating in bands of three block rows), vy a row profile
    (alternating in bands of three block columns); the steps are sized for the mask time of this blob's direction (256 - time256
    for the backward blob, time256 for the forward one)"""
    b = _fresh(blob)
    rng = np.random.default_rng(seed)
    xy, sad = records(b, ad)
    by, bx = sad.shape
    assert bx >= 14 and by >= 14, "the grid is too small for the profile"
    xmin, xmax, ymin, ymax = legal_rect(ad)
    mt = 256 - time256 if ad.isBackward else time256
    tx, ty, nx, ny = occlusion_terms(ad, mt, ml)
    cols = [_profile(bx, xmin, xmax, tx, nx, rng), np.zeros(bx, np.int64)]
    cols[1][1:] = _profile(bx - 1, xmin[1:], xmax[1:], tx, nx, rng, last_big=False)     # the same shifted by one column
    rows = [_profile(by, ymin, ymax, ty, ny, rng), np.zeros(by, np.int64)]
    rows[1][1:] = _profile(by - 1, ymin[1:], ymax[1:], ty, ny, rng, last_big=False)
    xy[:, :, 0] = np.stack([cols[(r // 3) % 2] for r in range(by)])
    xy[:, :, 1] = np.stack([rows[(c // 3) % 2] for c in range(bx)], axis=1)
    sad[:, :] = rng.integers(0, sad_max + 1, (by, bx))
    return b


def occlusion_stats(vx, vy, is_backward, ad, mask_time, ml):
    """what the steps of a field do in MakeVectorOcclusionMaskTime (MaskFun.cpp:106-129), both axes together: the largest span
    o * time4096 / 4096, the number of backward spans that max(0, ...) cuts, the number of ranges that end on the last block
    (nBlk - 1), the number of forward ranges that are empty (span >= 2: maxb < minb), and saturated / unsaturated value counts"""
    tx, ty, nx, ny = occlusion_terms(ad, mask_time, ml)
    st = dict(max_span=0, cut_first=0, at_last=0, empty=0, saturated=0, partial=0)
    for v, t, norm in ((np.asarray(vx, np.int64), tx, nx), (np.asarray(vy, np.int64).T, ty, ny)):
        n = v.shape[1]
        o = v[:, :-1] - v[:, 1:]
        pos = np.broadcast_to(np.arange(n - 1)[None, :], o.shape)[o > 0]
        o = o[o > 0]
        span = o * t // 4096
        val = np.minimum((255 * o * norm).astype(np.int64), 255)
        st["max_span"] = max(st["max_span"], int(span.max()) if span.size else 0)
        if is_backward:
            st["cut_first"] += int(np.count_nonzero(pos + 1 - span < 0))
            st["at_last"] += int(np.count_nonzero(pos + 1 == n - 1))
        else:
            st["empty"] += int(np.count_nonzero(pos + 1 - span < pos))
            st["at_last"] += int(np.count_nonzero(np.minimum(pos + 1 - span, n - 1) == n - 1))
        st["saturated"] += int(np.count_nonzero(val == 255))
        st["partial"] += int(np.count_nonzero((val > 0) & (val < 255)))
    return st


# ------------------------------------------------------------------ recipe dispatch shared by the CPU and the GPU tests

class Recipe:
    """name + parameters of one recipe; editor() binds it to the thresholds of the filter under test.  The i-th blob of a case is edited
    with seed + i, so that no two blobs of a case get the same field."""

    def __init__(self, name, seed, **kw):
        self.name, self.seed, self.kw = name, seed, kw

    def __repr__(self):
        return self.name + "".join("-%s%s" % (k, v) for k, v in sorted(self.kw.items()))

    def editor(self, thsad=400, thscd1=400, thscd2=130, time256=128, ml=100.0, th_scaled=None):
        """-> edit(blob, ad, index).  thsad / thscd1 / thscd2 are the arguments of the filter under test, scaled here the way the filter
        does for the blob's analysis data; th_scaled replaces the scaled thsad where a filter scales differently (Recalculate)."""
        kw = self.kw

        def edit(blob, ad, index=0):
            seed = self.seed + index
            th, s1, s2 = scaled_thresholds(ad, thsad, thscd1, thscd2)
            if th_scaled is not None:
                th = th_scaled
            sad_max = s1 if kw.get("sad") == "scd" else 64   # "scd": SADs up to thscd1 (never counted as a scene change), for the SAD masks
            if self.name == "limits":
                return limits(blob, ad, seed, margin=kw.get("margin", 0), sad_max=sad_max)
            if self.name == "sad_edges":
                return sad_edges(blob, ad, seed, th)
            if self.name == "scene_count":
                only = kw.get("only")                     # blob indices that get k + over; the others get k
                over = kw.get("over", 0) if only is None or index in only else 0
                return scene_count(blob, ad, seed, s1, s2 + over, th)
            if self.name == "occlusion":
                return occlusion(blob, ad, seed, kw.get("time256", time256), ml, sad_max=sad_max)
            if self.name == "invalid":
                only = kw.get("only")
                return invalid(blob, ad) if only is None or index in only else _fresh(blob)
            raise ValueError(self.name)
        return edit


def case_editor(consumer, recipe, kw, rc=None):
    """the editor of one listed case: consumer names the list, kw the filter's keyword arguments (whose defaults are the reference's),
    rc the oracle's Recalculate object.  Both test files build their fields through this."""
    scd = dict(thscd1=kw.get("thscd1", 400), thscd2=kw.get("thscd2", 130))
    if consumer == "degrain":
        thsad = kw.get("thsad", 400)
        return recipe.editor(thsad=kw.get("thsadc", thsad) if recipe.kw.get("which") == "chroma" else thsad, **scd)
    if consumer == "compensate":
        return recipe.editor(thsad=kw.get("thsad", 10000), **scd)
    if consumer == "blockfps":
        return recipe.editor(ml=kw.get("ml", 100.0), **scd)
    if consumer == "recalculate":
        return recipe.editor(th_scaled=recalculate_threshold(rc))
    if consumer == "flowinter":
        return recipe.editor(ml=kw.get("ml", 100.0), time256=flowinter_time256(kw), **scd)
    if consumer in ("flow", "flowblur"):
        return recipe.editor(**scd)
    raise ValueError(consumer)


R = Recipe
B84, B168, B80, B160 = dict(blksize=8, overlap=4), dict(blksize=16, overlap=8), dict(blksize=8, overlap=0), dict(blksize=16, overlap=0)
B3216 = dict(blksize=32, blksizev=16, overlap=16, overlapv=8)

# Every list below is shared by tests/test_vector_fields.py (the field is what it claims) and tests/test_gpu_vector_fields.py (parity).

DEGRAIN_CASES = [
    # w, h, bits, radius, super kwargs, analyse kwargs, degrain kwargs, recipe
    (206, 118, 8, 1, {}, B84, {}, R("limits", 1)),                                      # uncovered strips
    (206, 118, 16, 1, {}, B168, {}, R("limits", 11)),                                   # 16 bit: the shadow plane
    (544, 168, 8, 3, {}, B168, {}, R("limits", 21)),                                    # the plan tile of the cell kernel, three tile columns
    (200, 120, 16, 1, dict(pel=4), B80, {}, R("limits", 41)),                           # no overlap: the cell kernel
    (200, 120, 8, 1, dict(pel=1), dict(blksize=8, overlap=2), {}, R("limits", 51)),
    (256, 144, 16, 1, {}, B3216, {}, R("limits", 61)),
    (512, 384, 8, 1, {}, dict(blksize=64, overlap=32), {}, R("limits", 71)),            # big blocks: the per-sample gather
    (206, 118, 8, 1, {}, B84, {}, R("sad_edges", 81)),
    (128, 96, 16, 1, {}, B168, dict(thsadc=150), R("sad_edges", 91, which="chroma")),   # SADs around the chroma threshold
    (128, 96, 8, 1, {}, B80, dict(limit=3, limitc=5), R("sad_edges", 101)),
    (544, 168, 16, 3, {}, B168, dict(thsad=300), R("sad_edges", 111)),
    (206, 118, 8, 1, {}, B84, {}, R("scene_count", 121)),                               # count == thscd2: usable
    (206, 118, 8, 1, {}, B84, {}, R("scene_count", 131, over=1, only=(0,))),            # the backward blob one over: only mvfw is used
    (192, 112, 16, 1, {}, B160, {}, R("scene_count", 141, over=1)),
    (206, 118, 8, 1, {}, B84, {}, R("invalid", 151, only=(0,))),
    (128, 96, 16, 1, {}, B160, {}, R("invalid", 161)),
]

COMPENSATE_CASES = [
    # w, h, bits, super kwargs, analyse kwargs, compensate kwargs, field shift (None: fields=0), recipe
    (206, 118, 8, {}, B84, {}, None, R("limits", 201)),
    (192, 112, 16, dict(pel=4), B168, dict(time=40.0), None, R("limits", 211)),
    (200, 120, 8, {}, B80, {}, None, R("limits", 221)),
    (128, 96, 16, {}, B160, dict(time=75.0), None, R("limits", 231)),
    (206, 118, 8, {}, B84, dict(thsad=200), None, R("sad_edges", 241)),
    (192, 112, 16, {}, B160, dict(thsad=300), None, R("sad_edges", 251)),
    (206, 118, 8, {}, B84, {}, None, R("scene_count", 261)),
    (206, 118, 8, {}, B84, {}, None, R("scene_count", 271, over=1)),
    (206, 118, 8, {}, B84, {}, None, R("invalid", 281)),
    (128, 96, 8, dict(pel=2), B84, {}, 1, R("limits", 291, margin=1)),                  # fields=1: vy + pel / 2 stays legal
    (192, 112, 16, dict(pel=4), B168, {}, -2, R("limits", 301, margin=2)),
]

BLOCKFPS_CASES = [
    # w, h, bits, analyse kwargs (delta), blockfps kwargs (24 fps input), recipe
    (128, 96, 8, B84, dict(num=60, den=1, mode=0), R("occlusion", 401)),
    (206, 118, 8, B84, dict(num=60, den=1, mode=1), R("occlusion", 411)),
    (200, 120, 8, B80, dict(num=60, den=1, mode=2), R("occlusion", 421)),
    (128, 96, 16, B84, dict(num=60, den=1, mode=3, ml=40.0), R("occlusion", 431)),
    (240, 208, 16, B168, dict(num=48, den=1, mode=4), R("occlusion", 441)),
    (128, 96, 8, B84, dict(num=60, den=1, mode=5, ml=20.0), R("occlusion", 451)),
    # modes 6-8 build their masks from the SADs (MaskFun.cpp:133-166 MakeSADMaskTime): SADs up to thscd1, ml 20 so that some saturate
    (240, 208, 8, B168, dict(num=60, den=1, mode=6, ml=20.0), R("occlusion", 461, sad="scd")),
    (128, 96, 16, dict(blksize=8, overlap=2), dict(num=60, den=1, mode=7, ml=20.0), R("occlusion", 471, sad="scd")),
    (128, 96, 8, dict(B84, delta=2), dict(num=36, den=1, mode=8, ml=20.0), R("occlusion", 481, time256=64, sad="scd")),
    (206, 118, 8, B84, dict(num=60, den=1, mode=3), R("limits", 491)),
    (206, 118, 16, B84, dict(num=60, den=1, mode=6, ml=20.0), R("limits", 541, sad="scd")),
    (192, 112, 16, B160, dict(num=60, den=1, mode=0), R("limits", 501)),
    (128, 96, 8, dict(B84, delta=2), dict(num=36, den=1, mode=5), R("limits", 511)),
    (206, 118, 8, B84, dict(num=60, den=1), R("scene_count", 521)),
    (206, 118, 8, B84, dict(num=60, den=1), R("scene_count", 531, over=1)),
]

RECALC_CASES = [
    # bits, pel of the old vectors' super clip, pel of Recalculate's, old analyse kwargs, recalculate kwargs, recipe (on the old blob)
    (8, 2, 2, B168, dict(blksize=8, overlap=4, thsad=100, smooth=1), R("limits", 601)),          # finer grid
    (16, 2, 2, B168, dict(blksize=8, overlap=4, thsad=100, smooth=0), R("limits", 611)),
    (8, 2, 2, B84, dict(blksize=32, overlap=16, thsad=100, smooth=1), R("limits", 621)),         # coarser grid
    (8, 1, 2, B168, dict(blksize=8, overlap=4, thsad=100, smooth=1), R("limits", 631)),          # old pel 1 -> new pel 2
    (16, 4, 2, B84, dict(blksize=32, overlap=16, thsad=100, smooth=0), R("limits", 641)),        # old pel 4 -> new pel 2
    (8, 2, 2, dict(B168, divide=2), dict(blksize=8, overlap=4, thsad=100), R("limits", 651)),    # a divided old clip
    (8, 2, 2, B168, dict(blksize=8, overlap=4, thsad=100, smooth=1), R("sad_edges", 661)),
    (16, 2, 2, B84, dict(blksize=32, overlap=16, thsad=100, smooth=0), R("sad_edges", 671)),
]

FLOWINTER_CASES = [
    # fmt, w, h, bits, super kwargs, analyse kwargs, filter kwargs (fps = FlowFPS from 24/1, else FlowInter), recipe
    ("420", 206, 118, 8, {}, B84, dict(fps=1, num=48, mask=2), R("limits", 701)),                # nBlkXP > nBlkX
    ("420", 128, 96, 16, dict(pel=4), B84, dict(fps=1, num=60, mask=1), R("limits", 711)),
    ("444", 128, 96, 8, dict(pel=1), B84, dict(fps=1, num=60, mask=0), R("limits", 721)),
    ("422", 160, 96, 16, {}, B84, dict(time=50.0), R("limits", 731)),
    ("gray", 206, 118, 16, {}, B84, dict(time=33.0), R("limits", 741)),
    ("420", 206, 118, 8, {}, B84, dict(fps=1, num=48, mask=2), R("occlusion", 751)),
    ("420", 240, 208, 16, {}, B168, dict(fps=1, num=60, mask=1), R("occlusion", 761)),
    ("444", 128, 96, 8, dict(pel=4), B84, dict(fps=1, num=60, mask=2), R("occlusion", 771)),
    ("422", 160, 120, 8, dict(pel=1), B80, dict(time=50.0), R("occlusion", 781)),
    ("gray", 128, 96, 16, {}, B84, dict(fps=1, num=48, mask=0), R("occlusion", 791)),
    ("420", 206, 118, 8, {}, B84, dict(time=70.0), R("scene_count", 801)),
    ("420", 206, 118, 8, {}, B84, dict(time=70.0), R("scene_count", 811, over=1)),
    ("420", 206, 118, 16, {}, B84, dict(fps=1, num=60, mask=2), R("scene_count", 821)),
]

BW, FW = dict(isb=1), dict(isb=0)
FLOW_CASES = [
    # fmt, w, h, bits, super kwargs, analyse kwargs (isb), filter kwargs (fs = the jobs' field_shift), recipe
    ("420", 206, 118, 8, {}, dict(B84, **BW), dict(time=100.0), R("limits", 901)),
    ("420", 206, 118, 16, {}, dict(B84, **FW), dict(time=100.0, mode=1), R("limits", 911)),
    ("444", 128, 96, 8, dict(pel=4), dict(B84, **BW), dict(time=60.0, mode=1, fs=2), R("limits", 921, margin=2)),
    ("422", 160, 96, 16, {}, dict(B84, **FW), dict(time=100.0, fs=-1), R("limits", 931, margin=1)),
    ("gray", 128, 96, 8, dict(pel=1), dict(B80, **BW), dict(time=100.0, mode=1), R("limits", 941)),
    ("420", 206, 118, 8, {}, dict(B84, **BW), dict(time=100.0), R("scene_count", 951)),
    ("420", 206, 118, 8, {}, dict(B84, **FW), dict(time=100.0, mode=1), R("scene_count", 961, over=1)),
]

BLUR_CASES = [
    # fmt, w, h, bits, super kwargs, analyse kwargs, filter kwargs, recipe
    ("420", 206, 118, 8, {}, B84, dict(blur=200.0), R("limits", 1001)),
    ("420", 128, 96, 16, {}, B84, dict(blur=200.0, prec=3), R("limits", 1011)),
]

# the launch shapes of the benchmark differ from the small ones: Degrain3 at 4K 16 bit and FlowFPS at 1080p 8 bit, one output frame each
FULL_DEGRAIN = (3840, 2160, 16, 3, {}, B168, {}, R("limits", 1101))
FULL_FLOWFPS = ("420", 1920, 1080, 8, {}, B84, dict(fps=1, num=48, mask=2), R("limits", 1111))
