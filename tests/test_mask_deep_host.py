"""CPU tests of deep mv.Mask (mvx_mask_create_deep, masks of 9 to 16 bits): creation through the package with deep=True -- every message of
mvx_mask_create in its order, the format message of the library's own, out_bits; the expansion; the restatement tests/mask_deep_ref.py against
the 8-bit one; the conditions tests/mask_deep_cases.py puts on the inputs of the GPU cases; and the depth independence of kind 1, the one check
that does not rest on the restatement's own shift."""
import numpy as np
import pytest

import mask_cases as mc
import mask_deep_cases as dc
import mask_deep_ref
import mask_ref
import pipeline as pl
from test_mask_host import BLOCKS, FORMAT, GEOMETRY, _ad, _err

DEEP_FORMAT = "Mask: input clip must be Gray or YUV (4:2:0, 4:2:2, 4:4:0, 4:4:4) of 8 to 16 bits, with constant dimensions."


# ---------------------------------------------------------------- creation

def test_argument_checks_in_the_reference_order(mv):
    ad = _ad(mv)
    m = lambda **kw: mv.Mask(ad, kw.pop("w", 320), kw.pop("h", 192), deep=True, **kw)
    assert _err(lambda: m(gamma=-0.5)) == "Mask: gamma must not be negative."
    assert _err(lambda: m(kind=6)) == "Mask: kind must 0, 1, 2, 3, 4, or 5."
    assert _err(lambda: m(kind=-1)) == "Mask: kind must 0, 1, 2, 3, 4, or 5."
    assert _err(lambda: m(time=-0.5)) == "Mask: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: m(time=100.5)) == "Mask: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: m(ysc=256)) == "Mask: ysc must be between 0 and 255 (inclusive)."     # ysc stays in 8-bit units at every depth
    assert _err(lambda: m(ysc=256, bits=16)) == "Mask: ysc must be between 0 and 255 (inclusive)."
    assert _err(lambda: m(ysc=-1)) == "Mask: ysc must be between 0 and 255 (inclusive)."
    assert _err(lambda: m(thscd1=16321)) == "Mask: thscd1 can be at most 16320."
    for kw in (dict(bits=7), dict(bits=17), dict(bits=32), dict(subsampling=(2, 1)), dict(subsampling=(1, 2)), dict(bits=16, subsampling=(2, 2))):
        assert _err(lambda: m(**kw)) == DEEP_FORMAT, kw
    # the order: gamma, kind, time, ysc, the vector clip and thscd1, the format, then the library's own checks
    assert _err(lambda: m(gamma=-1.0, kind=9, time=200.0, ysc=999, thscd1=99999, bits=17)).startswith("Mask: gamma")
    assert _err(lambda: m(kind=9, time=200.0, ysc=999, thscd1=99999, bits=17)).startswith("Mask: kind")
    assert _err(lambda: m(time=200.0, ysc=999, thscd1=99999, bits=17)).startswith("Mask: time")
    assert _err(lambda: m(ysc=999, thscd1=99999, bits=17)).startswith("Mask: ysc")
    assert _err(lambda: m(thscd1=99999, bits=17)).startswith("Mask: thscd1")
    assert _err(lambda: m(bits=17, w=336)) == DEEP_FORMAT
    m(gamma=0.0, kind=5, time=0.0, ysc=255, thscd1=16320, bits=16)
    m(gamma=-0.0, kind=0, time=100.0, ysc=0, bits=9)
    m(gamma=-1e-60, bits=12)


def test_the_librarys_own_checks_still_come_last(mv):
    ad = _ad(mv)
    for bits in (8, 10, 16):
        assert _err(lambda: mv.Mask(ad, 336, 192, bits=bits, deep=True)) == GEOMETRY
        assert _err(lambda: mv.Mask(ad, 320, 192, bits=bits, subsampling=(0, 0), deep=True)) == GEOMETRY
        assert _err(lambda: mv.Mask(ad, 320, 192, bits=bits, gray=True, deep=True)) == GEOMETRY
        assert "multiples of 16" in _err(lambda: mv.Mask(ad, 320, 192, bits=bits, dst_pitch=[648, 320, 320], deep=True))
        assert "multiples of 16" in _err(lambda: mv.Mask(ad, 320, 192, bits=bits, dst_pitch=[640, 320, 336], deep=True))
    for w, h in ((8, 64), (64, 8)):
        tiny = mv.Analyse(mv.Super(w, h, 16), isb=1, blksize=8, overlap=0).ad
        assert _err(lambda: mv.Mask(tiny, w, h, bits=16, deep=True)) == BLOCKS
        assert _err(lambda: mv.Mask(tiny, w, h, bits=17, deep=True)) == DEEP_FORMAT    # the format check comes first
    gray = mv.Analyse(mv.Super(320, 192, 12, gray=True, subsampling=(0, 0)), isb=1).ad
    g = mv.Mask(gray, 320, 192, bits=12, gray=True, deep=True)                          # Gray in -> 4:4:4 out, at 12 bits
    assert (g.info.num_planes, g.info.subsampling_w, g.info.subsampling_h, g.out_bits) == (3, 0, 0, 12)
    assert list(g.info.plane_width) == [320] * 3 and list(g.info.plane_height) == [192] * 3


def test_without_the_argument_nothing_changes(mv):
    ad = _ad(mv)
    assert _err(lambda: mv.Mask(ad, 320, 192, bits=16)) == FORMAT
    assert _err(lambda: mv.Mask(ad, 320, 192, bits=16, deep=False)) == FORMAT
    plain = mv.Mask(ad, 320, 192)
    assert plain.out_bits == 8 and plain.pitch == [512, 256, 256]


def test_out_bits_pitches_and_info(mv):
    ad = _ad(mv)
    plain = mv.Mask(ad, 320, 192, kind=5, time=37.5, ml=3.0, gamma=0.7)
    for bits in range(8, 17):
        g = mv.Mask(ad, 320, 192, bits=bits, kind=5, time=37.5, ml=3.0, gamma=0.7, deep=True)
        assert g.out_bits == bits
        assert g.pitch == ([512, 256, 256] if bits == 8 else [768, 512, 512])             # bytes for the output depth, rounded up to 256
        assert bytes(g.info) == bytes(plain.info)                                          # the info describes samples: the same at every depth


# ---------------------------------------------------------------- the expansion

@pytest.mark.parametrize("s", range(9))
def test_expansion_endpoints_and_monotony(s):
    m = np.arange(256)
    w, o = mask_deep_ref.expand(m, s, True).astype(np.int64), mask_deep_ref.expand(m, s, False).astype(np.int64)
    peak = (1 << (8 + s)) - 1
    assert w[0] == 0 and w[255] == peak and np.all(np.diff(w) > 0) and w.max() <= peak          # a weight: 0 stays 0, full stays full
    assert o[0] == 0 and o[128] == 1 << (7 + s) and np.all(np.diff(o) == 1 << s) and o.max() <= peak   # an offset: 128 stays neutral
    assert np.array_equal(w >> s, m) and np.array_equal(o >> s, m)                              # the byte is the sample's high part
    if s == 0:
        assert np.array_equal(w, m) and np.array_equal(o, m)
    if s == 8:
        assert np.array_equal(w, m * 257)


# ---------------------------------------------------------------- the restatement against the 8-bit one

@pytest.mark.parametrize("case", [c for c in dc.CASES if c[6]["kind"] != 1], ids=dc.ids([c for c in dc.CASES if c[6]["kind"] != 1]))
def test_restatement_is_the_expanded_8_bit_restatement(oracle, case):
    """kinds 0, 2, 3, 4 and kind 5's chroma: E(8-bit restatement) sample for sample; kind 5's luma is the clip's own"""
    ad, blobs = dc.oracle_vectors(oracle, case)
    _, lumas = dc.frames_of(case)
    want, _, ref = dc.expected(case, ad, blobs, lumas)
    kind, s = case[6]["kind"], case[10] - 8
    low = mask_ref.Mask(ad, **case[6])
    dummy = np.zeros((case[2], case[1]), np.uint8)
    for n, b in enumerate(blobs):
        planes = low.frame(b, dummy if kind == 5 else None, {})
        for p in range(3):
            if kind == 5 and p == 0:
                assert np.array_equal(want[n][0], lumas[n]) and want[n][0].dtype == lumas[n].dtype
            else:
                assert np.array_equal(want[n][p], mask_deep_ref.expand(planes[p], s, kind <= 2)), (n, p)
            assert want[n][p].dtype == (np.uint8 if s == 0 else np.uint16) and int(want[n][p].max()) < 1 << case[10]


# ---------------------------------------------------------------- the GPU cases: what they cover and the conditions on their inputs

def _tail(w):
    return (w - 1) % 16 + 1


def test_cases_cover_what_the_feature_has():
    cases = dc.CASES + dc.FULL_CASES
    mk = [c[6] for c in cases]
    assert {c[10] for c in cases} == {8, 9, 10, 12, 14, 16} and all(c[3] == c[10] for c in cases)
    assert {k["kind"] for k in mk} == set(range(6))
    for kind in (0, 1, 2):
        gammas = {k.get("gamma", 1.0) for k in mk if k["kind"] == kind}
        assert 1.0 in gammas and len(gammas) > 1
    assert {c[0] for c in cases} == {"420", "422", "444", "gray"}
    blocks = {(c[0], c[5]["blksize"], c[5]["overlap"]) for c in cases}
    assert blocks >= {("420", 16, 8), ("420", 8, 4), ("420", 4, 2)}
    sub = lambda c: mc.FORMATS[c[0]].get("subsampling", (0, 0))
    sizes = {(c[1], c[2], c[0]) for c in cases}
    assert sizes >= {(128, 96, "420"), (206, 118, "420"), (137, 96, "444"), (144, 96, "420"), (130, 98, "420"), (1920, 1080, "420")}
    assert {_tail(c[1] >> sx) for c in cases for sx in (0, sub(c)[0])} >= {16, 14, 9, 8, 7, 2, 1}
    assert {(c[2] >> sy) % 4 for c in cases for sy in (0, sub(c)[1])} == {0, 1, 2, 3}
    forced = {c[6]["kind"] <= 2 for c in cases if c[6].get("thscd1") == 20}
    invalid = {c[6]["kind"] <= 2 for c in cases if c[7] is not None and c[7].name == "invalid"}
    assert forced == invalid == {True, False}                                                  # the fill in both expansion forms
    assert all(c[6].get("ysc", 0) > 0 for c in cases if c[6].get("thscd1") == 20 or (c[7] is not None and c[7].name == "invalid"))
    recipes = {(c[7].name, c[6]["kind"]) for c in cases if c[7] is not None}
    assert recipes >= {("limits", 0), ("limits", 3), ("limits", 5), ("sad_edges", 1), ("occlusion", 2)} and any(r[0] == "scene_count" for r in recipes)
    assert any(c[7] is not None and c[7].name == "sad_edges" and c[10] == 16 for c in cases)
    assert len({c[8] for c in cases}) == len(cases)


@pytest.mark.parametrize("case", dc.CASES + dc.FULL_CASES, ids=dc.ids(dc.CASES + dc.FULL_CASES))
def test_gpu_case_inputs_meet_the_conditions(oracle, case):
    """through the oracle's vectors: no 255 * pow(...) whose byte another pow could change lies within POW_MARGIN of the integer it must not
    cross; the case reaches the branches it claims; and a kind 1 case above 8 bits changes at least half of its cells by the shift"""
    ad, blobs = dc.oracle_vectors(oracle, case)
    _, lumas = dc.frames_of(case)
    _, kinds, ref = dc.expected(case, ad, blobs, lumas)
    print("pow distance %.3g, shifted %d of %d cells" % (ref.pow_dist, ref.shifted, ref.cells))
    assert ref.pow_dist >= dc.POW_MARGIN
    assert kinds == case[9]
    if case[6]["kind"] == 1 and "thscd1" not in case[6]:
        assert ref.cells > 0
        if case[10] > 8:
            assert 2 * ref.shifted >= ref.cells
        else:
            assert ref.shifted == 0
    if case[7] is not None and case[7].name == "sad_edges":
        assert max(int(pl.blob_vectors(b, ad)[2].max()) for b in blobs) > 2 ** 32           # crafted SADs above 2^32 must survive the shift


# ---------------------------------------------------------------- depth independence of kind 1

def independence_vectors(analyse_of, geo):
    """(ad, blob) of frame 0 against frame 1 (isb 1, pel 1) for the 8-bit clip and for the clip shifted left by s, with the premise asserted:
    identical vectors, SADs exactly 2^s times larger.  analyse_of(frames, bits) -> (ad, blob as numpy)"""
    s = geo[4] - 8
    low, high = dc.independence_clips(geo)
    (ad8, b8), (adB, bB) = analyse_of(low, 8), analyse_of(high, geo[4])
    x8, y8, sad8 = pl.blob_vectors(b8, ad8)
    xB, yB, sadB = pl.blob_vectors(bB, adB)
    assert np.array_equal(x8, xB) and np.array_equal(y8, yB), "the premise: identical vectors"
    assert np.array_equal(sad8.astype(np.int64) << s, sadB), "the premise: SADs exactly 2^s times larger"
    assert np.any(x8 != 0) and len(np.unique(sad8)) > 16
    return (ad8, b8), (adB, bB)


@pytest.mark.parametrize("geo", dc.INDEPENDENCE, ids=["%dx%d-%s-b%d" % (g[1], g[2], g[0], g[4]) for g in dc.INDEPENDENCE])
@pytest.mark.parametrize("mkw", [dict(kind=1), dict(kind=1, gamma=0.5, ml=30.0, time=37.5)], ids=["gamma1", "gamma0.5"])
def test_kind1_does_not_depend_on_the_depth(oracle, geo, mkw):
    """an 8-bit clip and the same clip with every sample shifted left by s give, at pel 1, identical vectors and SADs 2^s times larger; so the
    deep mask at depth 8 + s of the shifted clip is E(the 8-bit mask of the original), every sample"""
    fmt, w, h, akw, depth = geo

    def analyse_of(frames, bits):
        sup = oracle.Super(w, h, bits, pel=1, **mc.FORMATS[fmt])
        sf = [sup.frame(fr) for fr in frames]
        an = oracle.Analyse(sup, num_frames=mc.NF, isb=1, **akw)
        return an.ad, an.frame(sf[0], sf[1])

    (ad8, b8), (adB, bB) = independence_vectors(analyse_of, geo)
    low = mask_ref.Mask(ad8, **mkw).frame(b8, None, {})
    deep = mask_deep_ref.DeepMask(adB, depth, **mkw)
    high = deep.frame(bB, None, {})
    assert len(np.unique(low[0])) > 8
    for p in range(3):
        assert np.array_equal(high[p], mask_deep_ref.expand(low[p], depth - 8, True)), p
    assert 2 * deep.shifted >= deep.cells > 0
