"""CPU: the masked cases of tests/test_gpu_blockfps_float.py test what they claim.  The float clip's quantised copy is the integer clip
(degrain_float_cases.float_clip asserts it), so the vectors are the integer clip's; through the oracle's search alone, on every interpolated
output frame of each case at its ml: every mask the mode reads is above 0 on at least a tenth of the luma samples and below 255 on at least a
tenth.  A float BlockFPS that ignored its masks, or took them for saturated, could not pass those cases.  The same holds for the crafted fields
of the nine-mode cases, and the fallback cases are shown to be fallbacks: a scene change by one block too many, and a frame past the clip's end."""
import numpy as np
import pytest

import blockfps_float_cases as bc
import degrain_float_cases as fc
import degrain_n_cases as dc
import vector_fields

F = np.float32
_searches = {}


def _search(oracle, fmt, bits, blk, w, h, delta=1):
    key = (fmt, bits, blk[0], w, h, delta)
    if key not in _searches:
        frames = bc.int_clip(fmt, bits, w, h)
        fc.float_clip(frames[:1], bits, seed=9)  # (asserts that the quantised copy of the float clip is the integer clip)
        osup = oracle.Super(w, h, bits, **dict(dc.FORMATS[fmt], **blk[1]))
        osf = [osup.frame(f) for f in frames]
        abw, afw = oracle.Analyse(osup, num_frames=len(frames), isb=1, delta=delta, **blk[2]), oracle.Analyse(osup, num_frames=len(frames), isb=0, delta=delta, **blk[2])
        n = len(frames)
        bw = [abw.frame(osf[m], osf[m + delta] if m + delta < n else None) for m in range(n)]
        fw = [afw.frame(osf[m], osf[m - delta] if m >= delta else None) for m in range(n)]
        _searches[key] = (frames, osup, [[p.astype(F) for p in fr] for fr in osf], abw.ad, afw.ad, bw, fw)
    return _searches[key]


def _shares(oracle, s, bkw, bw, fw, gray):
    frames, osup, fsf, adb, adf, _, _ = s
    ob = oracle.BlockFPS(osup, adb, adf, len(frames), 24, 1, num=60, den=1, **bkw)
    ref = bc.restatement(oracle, adb, adf, bkw, gray=gray)
    clip = fc.integer_valued(frames)
    lo, hi, usable = 1.0, 1.0, 0
    for n in range(ob.num_frames):
        bc.want_frame(ref, ob.map, n, clip, fsf, bw, fw)
        if ref.masks is not None:
            a, b = bc.mask_shares(ref)
            lo, hi, usable = min(lo, a), min(hi, b), usable + 1
    return lo, hi, usable


@pytest.mark.parametrize("case", [c for c in bc.SEARCHED if c[5] >= 3], ids=bc.searched_id)
def test_searched_masks_are_neither_empty_nor_saturated(oracle, case):
    fmt, bits, blk, w, h, mode, ml = case
    s = _search(oracle, fmt, bits, blk, w, h)
    lo, hi, usable = _shares(oracle, s, dict(mode=mode, ml=ml), s[5], s[6], fmt == "gray")
    print("%s ml %g: above 0 on %.3f of the luma samples at least, below 255 on %.3f, %d interpolated frames" % (bc.searched_id(case), ml, lo, hi, usable))
    assert usable == 8 and lo >= bc.SHARE and hi >= bc.SHARE, (lo, hi, usable)


@pytest.mark.parametrize("mode", [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("geo", bc.MODES, ids=lambda g: bc.geo_id(*g[:5]))
def test_crafted_masks_are_neither_empty_nor_saturated(oracle, geo, mode):
    fmt, bits, blk, w, h, recipe = geo
    s = _search(oracle, fmt, bits, blk, w, h)
    bkw = dict(mode=mode, ml=bc.crafted_ml(recipe, mode))
    bw = [bc.crafted(recipe, b, s[3], 100 + m, bkw) if m + 1 < len(s[5]) else b for m, b in enumerate(s[5])]
    fw = [bc.crafted(recipe, b, s[4], 200 + m, bkw) if m >= 1 else b for m, b in enumerate(s[6])]
    lo, hi, usable = _shares(oracle, s, bkw, bw, fw, False)
    assert usable == 8 and lo >= bc.SHARE and hi >= bc.SHARE, (lo, hi, usable)


def test_the_fallback_cases_are_fallbacks(oracle):
    """one block too many above thscd1 makes a frame pair unusable and one fewer does not; with delta 2 the 24 -> 60 outputs 8 and 9 lie between
    frame 3 and a frame past the clip's end, at a time256 that is not 0"""
    fmt, bits, blk, w, h = bc.SMALL[0]
    frames, osup, fsf, adb, adf, bw, fw = _search(oracle, fmt, bits, blk, w, h)
    ref = bc.restatement(oracle, adb, adf, dict(mode=3))
    _, s1, s2 = vector_fields.scaled_thresholds(adb, 400)
    over, on = vector_fields.scene_count(bw[1], adb, 77, s1, s2 + 1, 400), vector_fields.scene_count(bw[1], adb, 77, s1, s2, 400)
    assert ref.usable(102, fsf[1], fsf[2], fw[2], on) and not ref.usable(102, fsf[1], fsf[2], fw[2], over)
    s = _search(oracle, fmt, bits, blk, w, h, delta=2)
    ob = oracle.BlockFPS(s[1], s[3], s[4], len(frames), 24, 1, num=60, den=1)
    assert [ob.map(n) for n in (8, 9)] == [(3, 5, 25), (3, 5, 77)] and ob.map(7) == (2, 4, 102)
