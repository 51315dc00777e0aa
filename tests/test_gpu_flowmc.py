"""GPU parity of mv.Flow / mv.FlowBlur (mvx_flow.hip) against the CPU restatement tests/flowmc_ref.py.  The restatement is fed the GPU's own
super frames (through mv.Finest's layout, mvoracle.Super.finest) and vectors, which other tests pin, so only the flow stage is compared.
Bit-exact; every output frame of each case in ONE *_frames call, mixing compensated and copied frames.

Each case names what its frames exercised: copy / fetch / shift / blur, and from the restatement's counters "collide" (a shift destination
that two or more sources with different samples reach: the last writer in raster order must win), "hole" (a destination no source reaches:
pixel_max), "taps" / "notaps" (FlowBlur samples with and without taps) and "trunc" (a negative v0 / m with a remainder: C's truncating
division)."""
import numpy as np
import pytest

import flowmc_ref
import pipeline as pl

pytestmark = pytest.mark.gpu

FORMATS = {"420": dict(subsampling=(1, 1)), "444": dict(subsampling=(0, 0)), "422": dict(subsampling=(1, 0)), "gray": dict(gray=True)}

B84, B168, B80 = dict(blksize=8, overlap=4), dict(blksize=16, overlap=8), dict(blksize=8, overlap=0)
BW, FW = dict(isb=1), dict(isb=0)
SH = "collide,copy,hole,shift"
FLOW_CASES = [
    # fmt, w, h, bits, super kwargs, analyse kwargs (isb, delta), filter kwargs (fs = the jobs' field_shift), what the frames exercised
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(time=100.0), "copy,fetch"),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(time=100.0, mode=1), SH),
    ("420", 128, 96, 8, {}, dict(B84, **FW), dict(time=50.0), "copy,fetch"),
    ("420", 128, 96, 8, {}, dict(B84, **FW), dict(time=37.5, mode=1), SH),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(time=0.0), "copy,fetch"),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(time=0.0, mode=1), "copy,shift"),                    # time256 0: the identity
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(time=0.39062499, mode=1), "copy,shift"),             # time256 0 in double (1 in float)
    ("420", 128, 96, 16, {}, dict(B84, isb=1, delta=2), dict(time=100.0), "copy,fetch"),
    ("420", 128, 96, 16, {}, dict(B84, isb=0, delta=2), dict(time=100.0, mode=1), SH),
    ("420", 128, 96, 8, {}, dict(B84, isb=0, delta=-2), dict(time=100.0), "fetch"),                     # absolute reference: frame 2
    ("420", 128, 96, 8, {}, dict(B84, isb=1, delta=-1), dict(time=80.0, mode=1), "collide,hole,shift"),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(time=100.0, fs=1), "copy,fetch"),                     # field_shift +pel/2
    ("420", 128, 96, 16, {}, dict(B84, **FW), dict(time=100.0, mode=1, fs=-1), SH),                    # field_shift -pel/2
    ("420", 128, 96, 8, dict(pel=4), dict(B84, **BW), dict(time=100.0, fs=-2), "copy,fetch"),
    ("420", 128, 96, 8, dict(pel=4), dict(B84, **FW), dict(time=60.0, mode=1, fs=2), SH),
    ("420", 128, 96, 8, dict(pel=1), dict(B84, **BW), dict(time=100.0), "copy,fetch"),
    ("420", 128, 96, 16, dict(pel=1), dict(B80, **BW), dict(time=100.0, mode=1), SH),
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(time=100.0, thscd1=20, thscd2=10), "copy"),          # scene change: the clip frame
    ("420", 128, 96, 8, {}, dict(B84, **BW), dict(time=100.0, mode=1, thscd1=20, thscd2=10), "copy"),
    ("420", 206, 118, 8, {}, dict(B84, **BW), dict(time=100.0), "copy,fetch"),                         # nBlkXP > nBlkX and nBlkYP > nBlkY
    ("420", 206, 118, 16, {}, dict(B84, **FW), dict(time=100.0, mode=1), SH),
    ("420", 192, 112, 8, {}, dict(B168, **BW), dict(time=75.0), "copy,fetch"),
    ("420", 192, 112, 16, {}, dict(B168, **BW), dict(time=100.0, mode=1), SH),
    ("420", 200, 120, 8, {}, dict(B80, **FW), dict(time=100.0, mode=1), SH),
    ("420", 160, 96, 8, {}, dict(blksize=16, blksizev=8, overlap=4, overlapv=2, isb=1), dict(time=100.0), "copy,fetch"),  # blksizev != blksize
    ("420", 160, 96, 8, {}, dict(blksize=16, blksizev=8, overlap=4, overlapv=2, isb=0), dict(time=100.0, mode=1), SH),
    ("444", 128, 96, 8, {}, dict(B84, **BW), dict(time=100.0), "copy,fetch"),
    ("444", 128, 96, 16, dict(pel=4), dict(B84, **FW), dict(time=100.0, mode=1), SH),
    ("422", 128, 96, 8, {}, dict(B84, **BW), dict(time=100.0, mode=1), SH),
    ("422", 160, 96, 16, {}, dict(B84, **FW), dict(time=100.0), "copy,fetch"),
    ("gray", 128, 96, 8, {}, dict(B84, **BW), dict(time=100.0, mode=1), SH),
    ("gray", 206, 118, 16, {}, dict(B84, **FW), dict(time=100.0), "copy,fetch"),
]
BLUR_CASES = [
    # fmt, w, h, bits, super kwargs, analyse kwargs, filter kwargs, what the frames exercised
    ("420", 128, 96, 8, {}, B84, dict(blur=50.0), "blur,copy,notaps,taps"),
    ("420", 128, 96, 8, {}, B84, dict(blur=0.0), "blur,copy,notaps"),
    ("420", 128, 96, 8, {}, B84, dict(blur=0.78124999), "blur,copy,notaps"),                         # blur256 1 in float (0 in double)
    ("420", 128, 96, 16, {}, B84, dict(blur=200.0), "blur,copy,taps,trunc"),
    ("420", 128, 96, 8, {}, B84, dict(blur=200.0, prec=3), "blur,copy,notaps,taps"),
    ("420", 128, 96, 16, {}, B84, dict(blur=200.0, prec=64), "blur,copy,notaps"),
    ("420", 128, 96, 8, {}, dict(B84, delta=2), dict(blur=150.0), "blur,copy,taps,trunc"),
    ("420", 128, 96, 8, {}, B84, dict(blur=50.0, thscd1=20, thscd2=10), "copy"),                     # scene change: the clip frame
    ("420", 206, 118, 8, {}, B84, dict(blur=120.0), "blur,copy,taps,trunc"),                  # the grid does not cover the frame
    ("420", 206, 118, 16, {}, B80, dict(blur=200.0), "blur,copy,taps,trunc"),
    ("420", 128, 96, 8, dict(pel=1), B84, dict(blur=200.0), "blur,copy,taps,trunc"),
    ("420", 128, 96, 16, dict(pel=4), B84, dict(blur=100.0), "blur,copy,taps,trunc"),
    ("420", 192, 112, 8, {}, B168, dict(blur=200.0), "blur,copy,taps,trunc"),
    ("420", 160, 96, 8, {}, dict(blksize=16, blksizev=8, overlap=4, overlapv=2), dict(blur=200.0), "blur,copy,taps,trunc"),
    ("444", 128, 96, 16, {}, B84, dict(blur=200.0), "blur,copy,taps,trunc"),
    ("422", 128, 96, 8, {}, B84, dict(blur=200.0, prec=3), "blur,copy,taps"),
    ("gray", 128, 96, 8, {}, B84, dict(blur=200.0), "blur,copy,taps,trunc"),
    ("gray", 206, 118, 16, dict(pel=4), B80, dict(blur=80.0), "blur,copy,taps,trunc"),
]


def _clip(mv, oracle, fmt, w, h, bits, skw, nf, seed, frames=None):
    """frames: the clip instead of moving_clip's (luma only for gray)"""
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
    widths = [gsup.info.plane_width[p] for p in range(gsup.nplanes)]
    finest = {}

    def fin(k):  # the Finest frame of the GPU's super frame k
        if k not in finest:
            finest[k] = osup.finest([mv.plane_to_numpy(gsf[k][p], widths[p], gsup.dtype) for p in range(gsup.nplanes)])
        return finest[k]
    return frames, gsup, gsrc, gsf, fin


def _kinds(kinds, stats):
    return ",".join(sorted(set(kinds) | {k for k, v in stats.items() if v > 0}))


def _compare(mv, out, want, k, n, kind):
    for p in range(len(want)):
        got = mv.plane_to_numpy(out[k][p], want[p].shape[1], want[p].dtype)
        assert np.array_equal(got, want[p]), "frame %d plane %d (%s): %s" % (n, p, kind, pl.first_diff(got, want[p]))


def _run_flow(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf, seed, outs=None, edit=None, frames=None):
    import torch
    frames, gsup, gsrc, gsf, fin = _clip(mv, oracle, fmt, w, h, bits, skw, nf, seed, frames=frames)
    akw, fkw = dict(akw), dict(fkw)
    isb, delta, fs = akw.pop("isb"), akw.pop("delta", 1), fkw.pop("fs", 0)
    ga = mv.Analyse(gsup, num_frames=nf, isb=isb, delta=delta, **akw)
    g = mv.Flow(gsup, ga.ad, nf, [p.stride(0) for p in gsrc[0]], **fkw)
    ref = flowmc_ref.Flow(ga.ad, nf, gsup.nplanes, gsup.info.hpad, gsup.info.vpad, bits, **fkw)
    inside = lambda k: 0 <= k < nf
    blobs = ga.run([(gsf[n], gsf[g.ref(n)] if inside(g.ref(n)) else None) for n in range(nf)])
    if edit is not None:  # replace the vectors of every blob (device copies)
        blobs = [torch.from_numpy(edit(b.cpu().numpy(), ga.ad)).to(b.device) for b in blobs]
    ns = list(range(nf)) if outs is None else outs
    for n in ns:
        assert g.ref(n) == ref.ref(n), n
    out = g.run([(gsrc[n], gsf[g.ref(n)] if inside(g.ref(n)) else None, blobs[n], fs) for n in ns])
    torch.cuda.synchronize()
    kinds, stats = set(), {}
    for k, n in enumerate(ns):
        want = ref.frame(n, frames, fin, blobs[n].cpu().numpy(), fs, stats)
        kinds.add(ref.last_kind)
        _compare(mv, out, want, k, n, ref.last_kind)
    return _kinds(kinds, stats)


def _run_blur(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf, seed, outs=None, edit=None, frames=None):
    import torch
    frames, gsup, gsrc, gsf, fin = _clip(mv, oracle, fmt, w, h, bits, skw, nf, seed, frames=frames)
    akw = dict(akw)
    delta = akw.pop("delta", 1)
    gabw = mv.Analyse(gsup, num_frames=nf, isb=1, delta=delta, **akw)
    gafw = mv.Analyse(gsup, num_frames=nf, isb=0, delta=delta, **akw)
    gbbw = gabw.run([(gsf[n], gsf[n + delta] if n + delta < nf else None) for n in range(nf)])
    gbfw = gafw.run([(gsf[n], gsf[n - delta] if n - delta >= 0 else None) for n in range(nf)])
    if edit is not None:
        gbbw = [torch.from_numpy(edit(b.cpu().numpy(), gabw.ad)).to(b.device) for b in gbbw]
        gbfw = [torch.from_numpy(edit(b.cpu().numpy(), gafw.ad)).to(b.device) for b in gbfw]
    g = mv.FlowBlur(gsup, gabw.ad, gafw.ad, nf, [p.stride(0) for p in gsrc[0]], **fkw)
    ref = flowmc_ref.FlowBlur(gabw.ad, gafw.ad, nf, gsup.nplanes, gsup.info.hpad, gsup.info.vpad, bits, **fkw)
    ns = list(range(nf)) if outs is None else outs
    out = g.run(ns, gsrc, gsf, gbbw, gbfw)
    torch.cuda.synchronize()
    bbw, bfw = [b.cpu().numpy() for b in gbbw], [b.cpu().numpy() for b in gbfw]
    kinds, stats = set(), {}
    for k, n in enumerate(ns):
        want = ref.frame(n, frames, fin, bbw, bfw, stats)
        kinds.add(ref.last_kind)
        _compare(mv, out, want, k, n, ref.last_kind)
    return _kinds(kinds, stats)


def test_cases_cover_every_path():
    """together the cases reach fetch, shift with colliding sources and holes, FlowBlur with and without taps and with truncating
    divisions, and the copies"""
    assert set(k for c in FLOW_CASES for k in c[-1].split(",")) == {"copy", "fetch", "shift", "collide", "hole"}
    assert set(k for c in BLUR_CASES for k in c[-1].split(",")) == {"copy", "blur", "taps", "notaps", "trunc"}


@pytest.mark.parametrize("fmt,w,h,bits,skw,akw,fkw,kinds", FLOW_CASES)
def test_flow_parity(oracle, mv, fmt, w, h, bits, skw, akw, fkw, kinds):
    assert _run_flow(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf=5, seed=101) == kinds


@pytest.mark.parametrize("fmt,w,h,bits,skw,akw,fkw,kinds", BLUR_CASES)
def test_flowblur_parity(oracle, mv, fmt, w, h, bits, skw, akw, fkw, kinds):
    """frames 0 and nf - 1 (delta 1) copy: mvbw at n - delta or mvfw at n + delta lies outside the clip"""
    assert _run_blur(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf=5, seed=103) == kinds


@pytest.mark.parametrize("w,h,bits,akw", [(1920, 1080, 8, B84), (3840, 2160, 16, B168)])
def test_flowmc_parity_full_size(oracle, mv, w, h, bits, akw):
    """Flow fetch, Flow shift and FlowBlur at the sizes users run: 1080p 8-bit and 4K 16-bit 4:2:0, output frame 1 of 3"""
    assert _run_flow(mv, oracle, "420", w, h, bits, {}, dict(akw, isb=1), dict(time=100.0), nf=3, seed=105, outs=[1]) == "fetch"
    assert _run_flow(mv, oracle, "420", w, h, bits, {}, dict(akw, isb=0), dict(time=100.0, mode=1), nf=3, seed=105, outs=[1]) == "collide,hole,shift"
    assert _run_blur(mv, oracle, "420", w, h, bits, {}, akw, dict(blur=50.0), nf=3, seed=105, outs=[1]) == "blur,notaps,taps"
