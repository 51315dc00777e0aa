"""GPU parity of deep mv.Mask (mvx_mask_create_deep: mask_planes_kernel<CLS, 1> and the shifted small-mask kernel of mvx_mask.hip) against the
CPU restatement tests/mask_deep_ref.py, through the Python package with deep=True.  The vectors come from the GPU's own Analyse, which other
tests pin; crafted fields are edited on the host and uploaded again.  Every sample of every plane of every frame, all frames of a case in ONE
mvx_mask_frames call.  The conditions of tests/mask_deep_cases.py are asserted on the vectors really used."""
import numpy as np
import pytest

import mask_cases as mc
import mask_deep_cases as dc
import mask_deep_ref
import pipeline as pl
from test_mask_deep_host import independence_vectors

pytestmark = pytest.mark.gpu


def _vectors(mv, case):
    """(Analyse, the clip's luma planes or None, their device frames or None, device blobs, the same blobs as numpy), edited by the case's recipe"""
    import torch
    fmt, w, h, bits, skw, akw = case[:6]
    frames, lumas = dc.frames_of(case)
    nf = mc.nf_of(case)
    gsup = mv.Super(w, h, bits, **dict(mc.FORMATS[fmt], **skw))
    gsf = gsup.build([mv.frame_to_device(fr) for fr in frames])
    ga = mv.Analyse(gsup, num_frames=nf, **akw)
    ref = [mc.reference_frame(n, akw["isb"], nf) for n in range(nf)]
    blobs = ga.run([(gsf[n], gsf[k] if k is not None else None) for n, k in enumerate(ref)])
    edit = mc.editor(case[:10], ga.ad)
    host = [edit(b.cpu().numpy(), n) for n, b in enumerate(blobs)]
    if case[7] is not None:
        blobs = [torch.from_numpy(e).to(b.device) for e, b in zip(host, blobs)]
    clip = [[mv.plane_to_device(l)] for l in lumas] if lumas is not None else None
    return ga, lumas, clip, blobs, host


def _mask(mv, case, ad, clip, deep=True, **extra):
    fmt, w, h = case[:3]
    f = mc.FORMATS[fmt]
    kw = dict(case[6], **extra)
    if clip is not None:
        kw["clip_pitch"] = [clip[0][0].stride(0)]
    return mv.Mask(ad, w, h, subsampling=f.get("subsampling", (1, 1)), gray=f.get("gray", False), bits=case[10] if deep else 8, deep=deep, **kw)


def _dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def _compare(mv, out, want, bits):
    for n, planes in enumerate(want):
        for p in range(3):
            got = mv.plane_to_numpy(out[n][p], planes[p].shape[1], _dtype(bits))
            assert got.shape == planes[p].shape and planes[p].dtype == got.dtype
            assert np.array_equal(got, planes[p]), "frame %d plane %d: %s" % (n, p, pl.first_diff(got, planes[p]))


def _run(mv, case):
    import torch
    ga, lumas, clip, blobs, host = _vectors(mv, case)
    g = _mask(mv, case, ga.ad, clip)
    assert g.out_bits == case[10]
    out = g.run(blobs, clip)
    torch.cuda.synchronize()
    want, kinds, ref = dc.expected(case, ga.ad, host, lumas)
    print("pow distance %.3g, shifted %d of %d cells" % (ref.pow_dist, ref.shifted, ref.cells))
    assert ref.pow_dist >= dc.POW_MARGIN, "the case's inputs do not meet the condition; give it another seed"
    if case[6]["kind"] == 1 and case[10] > 8:
        assert 2 * ref.shifted >= ref.cells > 0, "the shift would not show"
    _compare(mv, out, want, case[10])
    return kinds


@pytest.mark.parametrize("case", dc.CASES, ids=dc.ids(dc.CASES))
def test_deep_mask_parity(mv, case):
    assert _run(mv, case) == case[9]


@pytest.mark.parametrize("case", dc.FULL_CASES, ids=dc.ids(dc.FULL_CASES))
def test_deep_mask_parity_full_size(mv, case):
    """1920 x 1080 4:2:0 at 16 bits: the launch shape tools/mask_bench.py --bits 16 measures"""
    assert _run(mv, case) == case[9]


@pytest.mark.parametrize("seed", [311, 316])
def test_deep_output_is_the_expanded_8_bit_output(mv, seed):
    """kind 0 (a weight) and kind 5 (offsets): the deep object's planes equal E(the plain 8-bit Mask's planes) on the same device blobs"""
    import torch
    case = next(c for c in dc.CASES if c[8] == seed)
    kind, s = case[6]["kind"], case[10] - 8
    assert kind in (0, 5) and s > 0
    ga, lumas, clip, blobs, _ = _vectors(mv, case)
    deep = _mask(mv, case, ga.ad, clip).run(blobs, clip)
    low_luma = [[mv.plane_to_device((l >> s).astype(np.uint8))] for l in lumas] if lumas is not None else None   # (kind 5's luma is not compared)
    plain = _mask(mv, case, ga.ad, low_luma, deep=False).run(blobs, low_luma)
    torch.cuda.synchronize()
    for n in range(len(blobs)):
        for p in range(3):
            w = [case[1], case[1] // 2, case[1] // 2][p]
            got = mv.plane_to_numpy(deep[n][p], w, np.uint16)
            if kind == 5 and p == 0:
                assert np.array_equal(got, lumas[n])
            else:
                assert np.array_equal(got, mask_deep_ref.expand(mv.plane_to_numpy(plain[n][p], w, np.uint8), s, kind <= 2)), (n, p)


@pytest.mark.parametrize("geo", dc.INDEPENDENCE, ids=["%dx%d-%s-b%d" % (g[1], g[2], g[0], g[4]) for g in dc.INDEPENDENCE])
def test_kind1_does_not_depend_on_the_depth(mv, geo):
    """the GPU's own Analyse at pel 1 on an 8-bit clip and on the clip shifted left by s: identical vectors, SADs 2^s times larger (asserted);
    then the deep kind 1 mask of the shifted clip is E(the plain 8-bit mask of the original).  No restatement takes part."""
    import torch
    fmt, w, h, akw, depth = geo
    f = mc.FORMATS[fmt]
    dev = {}

    def analyse_of(frames, bits):
        sup = mv.Super(w, h, bits, pel=1, **f)
        sf = sup.build([mv.frame_to_device(fr) for fr in frames])
        an = mv.Analyse(sup, num_frames=mc.NF, isb=1, **akw)
        dev[bits] = (an.ad, an.run([(sf[0], sf[1])]))
        return an.ad, dev[bits][1][0].cpu().numpy()

    independence_vectors(analyse_of, geo)
    mkw = dict(kind=1, gamma=0.5, ml=30.0, time=37.5)
    low = mv.Mask(dev[8][0], w, h, subsampling=f["subsampling"], **mkw).run(dev[8][1])
    high = mv.Mask(dev[depth][0], w, h, subsampling=f["subsampling"], bits=depth, deep=True, **mkw).run(dev[depth][1])
    torch.cuda.synchronize()
    for p in range(3):
        pw = w >> (f["subsampling"][0] if p else 0)
        a = mv.plane_to_numpy(low[0][p], pw, np.uint8)
        assert p or len(np.unique(a)) > 8
        assert np.array_equal(mv.plane_to_numpy(high[0][p], pw, np.uint16), mask_deep_ref.expand(a, depth - 8, True)), p


@pytest.mark.parametrize("seed", [308, 339])
def test_deep_entry_at_8_bits_gives_the_plain_planes(mv, seed):
    """kind 1 and kind 5: byte for byte the plain object's planes, pitch bytes included"""
    import torch
    case = next(c for c in dc.CASES if c[8] == seed)
    assert case[10] == 8
    ga, lumas, clip, blobs, _ = _vectors(mv, case)
    a, b = _mask(mv, case, ga.ad, clip), _mask(mv, case, ga.ad, clip, deep=False)
    assert a.out_bits == b.out_bits == 8 and a.pitch == b.pitch
    outs = []
    for g in (a, b):
        out = [[torch.full((g.info.plane_height[p], g.pitch[p]), 0xA5, dtype=torch.uint8, device="cuda") for p in range(3)] for _ in blobs]
        g.run(blobs, clip, out=out)
        outs.append(out)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for fa, fb in zip(*outs) for x, y in zip(fa, fb))
    assert any(bool((x[:, :case[1] // 2] != 0xA5).any()) for fa in outs[0] for x in fa)


@pytest.mark.parametrize("seed", [316, 313, 333, 302, 314])
def test_only_the_samples_are_written_and_no_frames_is_a_no_op(mv, seed):
    """canary pitches at 206 x 118 (row tails of 14 and 7 samples) and 130 x 98 (2 and 1): the bytes of dst beyond each plane's width x 2 keep their
    value, for usable frames, for a NULL blob and for the fill; a call with nframes = 0 writes nothing"""
    import torch
    case = next(c for c in dc.CASES if c[8] == seed)
    assert (case[1], case[2]) in ((206, 118), (130, 98)) and case[0] == "420" and case[10] > 8
    ga, lumas, clip, blobs, host = _vectors(mv, case)
    pitch = [(case[1] * 2 + 15) // 16 * 16 + 16, (case[1] + 15) // 16 * 16 + 16, (case[1] + 15) // 16 * 16 + 16]   # a whole vector of canary bytes behind every row
    g = _mask(mv, case, ga.ad, clip, dst_pitch=pitch)
    blobs, host = list(blobs) + [None], list(host) + [None]
    if clip is not None:
        clip, lumas = clip + [clip[0]], lumas + [lumas[0]]
    n = len(blobs)
    out = [[torch.full((g.info.plane_height[p], g.pitch[p]), 0xA5, dtype=torch.uint8, device="cuda") for p in range(3)] for _ in range(n)]
    g.launch((mv.MaskJob * 0)())
    torch.cuda.synchronize()
    assert all(bool((pln == 0xA5).all()) for fr in out for pln in fr), "nframes = 0 wrote something"
    g.run(blobs, clip, out=out)
    torch.cuda.synchronize()
    ref = mask_deep_ref.DeepMask(ga.ad, case[10], **case[6])
    stats = {}
    for k in range(n):
        want = ref.frame(host[k], lumas[k] if lumas is not None else None, stats)
        for p in range(3):
            full = out[k][p].cpu().numpy()
            w = want[p].shape[1]
            got = np.ascontiguousarray(full[:, :2 * w]).view(np.uint16)
            assert np.array_equal(got, want[p]), "frame %d plane %d: %s" % (k, p, pl.first_diff(got, want[p]))
            assert full.shape[1] > 2 * w and np.all(full[:, 2 * w:] == 0xA5), "frame %d plane %d: bytes beyond the samples were written" % (k, p)
    assert stats["sc"] == 2 and stats["edgex"] > 0
