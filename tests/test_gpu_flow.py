"""GPU parity of mv.FlowInter / mv.FlowFPS (mvx_flow.hip) against the CPU restatement tests/flow_ref.py.  flow_ref is fed the GPU's own
super frames (through mv.Finest's layout, mvoracle.Super.finest) and vectors, which other tests pin, so only the flow stage is compared.
Bit-exact; every output frame of each case in ONE mvx_flow_frames call, mixing interpolated, Blend and copy jobs."""
import numpy as np
import pytest

import flow_ref
import pipeline as pl
import vector_fields

pytestmark = pytest.mark.gpu

FORMATS = {"420": dict(subsampling=(1, 1)), "444": dict(subsampling=(0, 0)), "422": dict(subsampling=(1, 0)), "gray": dict(gray=True)}

B84, B168, B80 = dict(blksize=8, overlap=4), dict(blksize=16, overlap=8), dict(blksize=8, overlap=0)
CASES = [
    # fmt, w, h, bits, super kwargs, analyse kwargs, filter kwargs (fps = FlowFPS from 24/1, else FlowInter), what the output frames take:
    # the formulas ("128": at time256 128, where Simple has its own), Blend, the left frame or FlowFPS's copy
    ("420", 128, 96, 8, {}, B84, dict(fps=1, num=48, mask=2), "copy,extra128,simple128"),
    ("420", 128, 96, 8, {}, B84, dict(fps=1, num=48, mask=1), "copy,regular128"),
    ("420", 128, 96, 8, {}, B84, dict(fps=1, num=48, mask=0), "copy,simple128"),
    ("420", 128, 96, 8, {}, B84, dict(fps=1, num=60, mask=2), "copy,extra,simple"),
    ("420", 128, 96, 8, {}, B84, dict(fps=1, num=60, mask=1), "copy,regular"),
    ("420", 128, 96, 8, {}, B84, dict(fps=1, num=60, mask=0), "copy,simple"),
    ("420", 128, 96, 16, {}, B84, dict(fps=1, num=48, mask=2), "copy,extra128,simple128"),
    ("420", 128, 96, 16, {}, B168, dict(fps=1, num=60, mask=1), "copy,regular"),
    ("420", 192, 112, 16, {}, B168, dict(fps=1, num=60, mask=0), "copy,simple"),
    ("420", 128, 96, 8, dict(pel=1), B84, dict(fps=1, num=48, mask=2), "copy,extra128,simple128"),
    ("420", 128, 96, 8, dict(pel=4), B84, dict(fps=1, num=60, mask=2), "copy,extra,simple"),
    ("420", 128, 96, 16, dict(pel=4), B80, dict(fps=1, num=48, mask=1), "copy,regular128"),
    ("420", 200, 120, 8, {}, B80, dict(fps=1, num=60, mask=2), "copy,extra,simple"),
    ("420", 206, 118, 8, {}, B84, dict(fps=1, num=60, mask=2), "copy,extra,simple"),                 # nBlkXP > nBlkX and nBlkYP > nBlkY
    ("420", 204, 124, 16, {}, B80, dict(fps=1, num=48, mask=0), "copy,simple128"),               # padded small fields, no overlap
    ("420", 160, 96, 8, {}, dict(blksize=16, blksizev=8, overlap=4, overlapv=2), dict(fps=1, num=60, mask=2), "copy,extra,simple"),  # blksizev != blksize
    ("420", 128, 96, 8, {}, dict(B84, delta=2), dict(fps=1, num=48, mask=2), "blend,copy,simple"),  # delta 2: time256 / 2, nright past the end
    ("420", 128, 96, 8, {}, B84, dict(fps=1, num=60, mask=2, thscd1=20, thscd2=10), "blend,copy"),           # scene change: Blend
    ("420", 128, 96, 8, {}, B84, dict(fps=1, num=60, mask=2, thscd1=20, thscd2=10, blend=0), "copy,left"),  # scene change: left frame
    ("420", 128, 96, 16, {}, B84, dict(fps=1, num=0, den=0, mask=2, ml=40.0), "copy,extra128,simple128"),  # default rate: double
    ("444", 128, 96, 8, {}, B84, dict(fps=1, num=48, mask=2), "copy,extra128,simple128"),
    ("444", 128, 96, 16, {}, B168, dict(fps=1, num=60, mask=1), "copy,regular"),
    ("422", 128, 96, 8, {}, B84, dict(fps=1, num=60, mask=0), "copy,simple"),
    ("422", 160, 96, 16, {}, B84, dict(fps=1, num=48, mask=2), "copy,extra128,simple128"),
    ("gray", 128, 96, 8, {}, B84, dict(fps=1, num=60, mask=2), "copy,extra,simple"),
    ("gray", 128, 96, 16, {}, B80, dict(fps=1, num=48, mask=1), "copy,regular128"),
    ("420", 128, 96, 8, {}, B84, dict(time=50.0), "blend,extra128,regular128"),
    ("420", 128, 96, 8, {}, B84, dict(time=0.0), "blend,extra,regular"),                              # no copy shortcut at time 0
    ("420", 128, 96, 8, {}, B84, dict(time=100.0), "blend,extra,regular"),
    ("420", 128, 96, 8, {}, B84, dict(time=0.39062499), "blend,extra,regular"),                       # time256 1 in float (0 in double)
    ("420", 128, 96, 16, {}, B168, dict(time=33.0, ml=33.3), "blend,extra,regular"),
    ("420", 128, 96, 8, {}, B84, dict(time=70.0, thscd1=20, thscd2=10), "blend"),
    ("420", 128, 96, 8, {}, B84, dict(time=70.0, thscd1=20, thscd2=10, blend=0), "left"),
    ("444", 128, 96, 16, dict(pel=4), B84, dict(time=25.0), "blend,extra,regular"),
    ("422", 200, 120, 8, dict(pel=1), B80, dict(time=60.0), "blend,extra,regular"),
    ("gray", 206, 118, 16, {}, B84, dict(time=45.0), "blend,extra,regular"),
]


def _run(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf, seed, outs=None, edit=None, ml_double=None, frames=None):
    """frames: the clip instead of moving_clip's (luma only for gray)"""
    import torch
    f = FORMATS[fmt]
    if frames is None:
        frames = pl.moving_clip(w, h, bits, nf, seed=seed, noise=3, sub=f.get("subsampling", (1, 1)))
        if f.get("gray"):
            frames = [[fr[0]] for fr in frames]
    assert len(frames) == nf and len(frames[0]) == (1 if f.get("gray") else 3)
    kw = dict(f, **skw)
    osup, gsup = oracle.Super(w, h, bits, **kw), mv.Super(w, h, bits, **kw)
    gsrc = [mv.frame_to_device(fr) for fr in frames]
    gsf = gsup.build(gsrc)
    akw = dict(akw)
    delta = akw.pop("delta", 1)
    gabw = mv.Analyse(gsup, num_frames=nf, isb=1, delta=delta, **akw)
    gafw = mv.Analyse(gsup, num_frames=nf, isb=0, delta=delta, **akw)
    gbbw = gabw.run([(gsf[n], gsf[n + delta] if n + delta < nf else None) for n in range(nf)])
    gbfw = gafw.run([(gsf[n], gsf[n - delta] if n - delta >= 0 else None) for n in range(nf)])
    if edit is not None:  # replace the vectors of every blob (device copies)
        gbbw = [torch.from_numpy(edit(b.cpu().numpy(), gabw.ad)).to(b.device) for b in gbbw]
        gbfw = [torch.from_numpy(edit(b.cpu().numpy(), gafw.ad)).to(b.device) for b in gbfw]
    fkw = dict(fkw)
    pitch = [p.stride(0) for p in gsrc[0]]
    if fkw.pop("fps", None):
        g = mv.FlowFPS(gsup, gabw.ad, gafw.ad, nf, pitch, 24, 1, **fkw)
        ref = flow_ref.Flow(gabw.ad, gafw.ad, nf, gsup.nplanes, gsup.info.hpad, gsup.info.vpad, fps=(24, 1), **fkw)
        assert (g.num_frames, g.fps_num, g.fps_den) == (ref.num_frames,) + ref.fps
    else:
        g = mv.FlowInter(gsup, gabw.ad, gafw.ad, nf, pitch, **fkw)
        ref = flow_ref.Flow(gabw.ad, gafw.ad, nf, gsup.nplanes, gsup.info.hpad, gsup.info.vpad, **fkw)
        assert g.num_frames == nf
    ns = list(range(g.num_frames)) if outs is None else outs
    for n in ns:
        assert g.map(n) == ref.map(n), n
    out = g.run(ns, gsrc, gsf, gbbw, gbfw)
    torch.cuda.synchronize()
    widths = [gsup.info.plane_width[p] for p in range(gsup.nplanes)]
    sup_np = lambda k: [mv.plane_to_numpy(gsf[k][p], widths[p], gsup.dtype) for p in range(gsup.nplanes)]
    finest = {}

    def fin(k):
        if k not in finest:
            finest[k] = osup.finest(sup_np(k))
        return finest[k]

    bbw, bfw = [b.cpu().numpy() for b in gbbw], [b.cpu().numpy() for b in gbfw]
    kinds, differs = set(), 0
    ref_d = None
    if ml_double is not None:  # the same filter with ml as a double: must give other masks, so that the case can tell the two apart
        ref_d = flow_ref.Flow(gabw.ad, gafw.ad, nf, gsup.nplanes, gsup.info.hpad, gsup.info.vpad, **fkw)
        ref_d.ml = ml_double
        assert ref_d.ml != ref.ml
    for k, n in enumerate(ns):
        want = ref.frame(n, frames, fin, bbw, bfw)
        kinds.add(ref.last_kind)
        for p in range(gsup.nplanes):
            got = mv.plane_to_numpy(out[k][p], want[p].shape[1], want[p].dtype)
            assert np.array_equal(got, want[p]), "frame %d plane %d %s (%s): %s" % (n, p, g.map(n), ref.last_kind, pl.first_diff(got, want[p]))
        if ref_d is not None:
            differs += sum(int(np.count_nonzero(a != b)) for a, b in zip(want, ref_d.frame(n, frames, fin, bbw, bfw)))
    if ref_d is not None:
        assert differs > 0, "the case does not separate float from double ml"
    return ",".join(sorted(kinds))


def test_cases_cover_every_formula():
    """together the cases reach each formula (Simple, regular and Extra, at time256 128 and elsewhere) and each fallback"""
    seen = set(k for c in CASES for k in c[-1].split(","))
    assert seen == {"simple", "simple128", "regular", "regular128", "extra", "extra128", "blend", "left", "copy"}


@pytest.mark.parametrize("fmt,w,h,bits,skw,akw,fkw,kinds", CASES)
def test_flow_parity(oracle, mv, fmt, w, h, bits, skw, akw, fkw, kinds):
    assert _run(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf=6, seed=91) == kinds


@pytest.mark.parametrize("w,h,bits,akw", [(1920, 1080, 8, B84), (3840, 2160, 16, B168)])
def test_flow_parity_full_size(oracle, mv, w, h, bits, akw):
    """FlowFPS 2x, mask=2 at the sizes users run: 1080p 8-bit and 4K 16-bit 4:2:0.  Output 1 lies in (0, 1), where mvfw at 0 is the invalid
    default blob (Simple); output 3 in (1, 2), where all four blobs are usable (Extra)"""
    assert _run(mv, oracle, "420", w, h, bits, {}, akw, dict(fps=1, num=48, mask=2), nf=4, seed=93, outs=[1, 3]) == "extra128,simple128"


def _alternating_vectors(o):
    """blob editor: level-0 vectors (0, 0) in even block columns and (-o, 0) in odd ones, SAD 0 -- an occlusion of o at every even column"""
    def edit(blob, ad):
        b = blob.copy()
        xy, sad = vector_fields.records(b, ad)
        xy[:, :, 0] = np.where(np.arange(xy.shape[1]) % 2 == 1, -o, 0)[None, :]
        xy[:, :, 1] = 0
        sad[:, :] = 0
        return b
    return edit


def test_flowinter_ml_reaches_the_mask_as_float(oracle, mv):
    """MVFlowInter.c:46-47,485-487: ml is a float argument.  At ml = 2550 / 21 an occlusion of one half-pel step over 4-sample block steps
    gives the mask value (int)(255 * 80 / (ml * 4 * 2)) = 20 with (double)(float)ml but 21 with the double"""
    ml = 2550.0 / 21
    assert _run(mv, oracle, "420", 128, 96, 8, {}, B84, dict(time=50.0, ml=ml), nf=3, seed=95, edit=_alternating_vectors(1), ml_double=ml) == "blend,regular128"
