"""GPU parity of mv.Mask (mvx_mask.hip) against the CPU restatement tests/mask_ref.py, through the Python package.  The vectors come from the
GPU's own Analyse, which other tests pin; crafted fields (tests/vector_fields.py) are edited on the host and uploaded again.  Bit-exact,
every sample of every plane; all frames of a case in ONE mvx_mask_frames call, mixing usable frames and frames filled with ysc.

Each case names what the restatement's counters saw (tests/mask_ref.py), so that it cannot pass without reaching its branch, and must meet
the condition of tests/mask_cases.py on its inputs: where the exponent is not 1, no 255 * pow(...) within POW_MARGIN of an integer."""
import numpy as np
import pytest

import mask_cases as mc
import mask_ref
import pipeline as pl

pytestmark = pytest.mark.gpu


def _vectors(mv, case):
    """(Analyse, the device frames of the 8-bit clip argument or None, device blobs, the same blobs as numpy), edited by the case's recipe"""
    import torch
    fmt, w, h, bits, skw, akw, mkw, _, _, _ = case
    frames, lumas = mc.frames_of(case)
    nf = mc.nf_of(case)
    gsup = mv.Super(w, h, bits, **dict(mc.FORMATS[fmt], **skw))
    gsf = gsup.build([mv.frame_to_device(fr) for fr in frames])
    ga = mv.Analyse(gsup, num_frames=nf, **akw)
    ref = [mc.reference_frame(n, akw["isb"], nf) for n in range(nf)]
    blobs = ga.run([(gsf[n], gsf[k] if k is not None else None) for n, k in enumerate(ref)])
    edit = mc.editor(case, ga.ad)
    host = [edit(b.cpu().numpy(), n) for n, b in enumerate(blobs)]
    if case[7] is not None:
        blobs = [torch.from_numpy(e).to(b.device) for e, b in zip(host, blobs)]
    clip = [[mv.plane_to_device(l)] for l in lumas] if lumas is not None else None
    return ga, lumas, clip, blobs, host


def _mask(mv, case, ad, clip, **extra):
    fmt, w, h = case[:3]
    f = mc.FORMATS[fmt]
    kw = dict(case[6], **extra)
    if clip is not None:
        kw["clip_pitch"] = [clip[0][0].stride(0)]
    return mv.Mask(ad, w, h, subsampling=f.get("subsampling", (1, 1)), gray=f.get("gray", False), **kw)


def _run(mv, case):
    import torch
    ga, lumas, clip, blobs, host = _vectors(mv, case)
    g = _mask(mv, case, ga.ad, clip)
    out = g.run(blobs, clip)
    torch.cuda.synchronize()
    want, kinds, dist = mc.expected(case, ga.ad, host, lumas)
    print("pow distance %.3g" % dist)
    assert dist >= mc.POW_MARGIN, "the case's inputs do not meet the condition; give it another seed"
    for n, planes in enumerate(want):
        for p in range(3):
            got = mv.plane_to_numpy(out[n][p], planes[p].shape[1], np.uint8)
            assert got.shape == planes[p].shape
            assert np.array_equal(got, planes[p]), "frame %d plane %d: %s" % (n, p, pl.first_diff(got, planes[p]))
    return kinds


@pytest.mark.parametrize("case", mc.CASES, ids=mc.ids(mc.CASES))
def test_mask_parity(mv, case):
    assert _run(mv, case) == case[-1]


@pytest.mark.parametrize("case", mc.FULL_CASES, ids=mc.ids(mc.FULL_CASES))
def test_mask_parity_full_size(mv, case):
    """1920 x 1080 4:2:0: the launch shape tools/mask_bench.py measures"""
    assert _run(mv, case) == case[-1]


@pytest.mark.parametrize("kind", [0, 5])
def test_only_the_samples_are_written_and_no_frames_is_a_no_op(mv, kind):
    """a canary pitch: the bytes of dst beyond each plane's width keep their value (206 and 103 leave row tails of 14 and 7 bytes: every
    narrow store), for usable frames, for a NULL blob and for the scene-change fill; a call with nframes = 0 writes nothing"""
    import torch
    case = next(c for c in mc.CASES if c[6]["kind"] == kind and (c[1], c[2]) == (206, 118) and c[0] == "420" and c[7] is None)
    ga, lumas, clip, blobs, host = _vectors(mv, case)
    g = _mask(mv, case, ga.ad, clip, dst_pitch=[224, 128, 128])
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
    ref = mask_ref.Mask(ga.ad, **case[6])
    stats = {}
    for k in range(n):
        want = ref.frame(host[k], lumas[k] if lumas is not None else None, stats)
        for p in range(3):
            full = out[k][p].cpu().numpy()
            w = want[p].shape[1]
            assert np.array_equal(full[:, :w], want[p]), "frame %d plane %d: %s" % (k, p, pl.first_diff(full[:, :w], want[p]))
            assert np.all(full[:, w:] == 0xA5), "frame %d plane %d: bytes beyond the width were written" % (k, p)
    assert stats["sc"] == 2 and stats["edgex"] > 0
