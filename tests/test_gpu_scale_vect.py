"""ScaleVect on the GPU (include/mvtools_amd.h, mv.ScaleVect; csrc/mvx_scale_vect.hip): for every case of tests/scale_vect_cases.py the scaled
blob is first compared byte for byte with the restatement (tests/scale_vect_ref.py), and only then handed to the existing consumers at
full size -- Degrain (radius 1), Compensate, and Recalculate with half the block size -- whose results must be the oracle's on the
restatement's blob and analysis data, byte for byte.  So the scaled data is a vector clip the whole pipeline accepts.

The small clip is the suite's synthetic clip (tests/synth.py; the formats it does not make come from tests/pipeline.py); the full-size
clip is another clip of scale times its size: byte parity needs no real motion.  tests/test_scale_vect_host.py checks the analysis data,
the restatement and the input of the end-to-end case on the CPU."""
import numpy as np
import pytest

import pipeline as pl
import scale_vect_cases as sc
import scale_vect_ref as ref
import synth

pytestmark = pytest.mark.gpu

ids = [c.name for c in sc.CASES]


def _frames(case, w, h, bits, n, small):
    if small and case.fmt in ("420", "gray"):
        frames = synth.survey_clip(w, h, bits, n)
    else:
        frames = pl.moving_clip(w, h, bits, n, seed=31, noise=3, sub=sc.SUB[case.fmt].get("subsampling", (1, 1)))
    return [[f[0]] for f in frames] if case.fmt == "gray" else frames


def _fields(ad):
    return {k: getattr(ad, k) for k, _ in ad._fields_}


def _upload(e, device):
    import torch
    return torch.from_numpy(e).to(device)


def _small(mv, case, n):
    (w, h), _ = sc.sizes(case)
    gsup = mv.Super(w, h, case.bits, **sc.super_kwargs(case, False))
    gsf = gsup.build([mv.frame_to_device(f) for f in _frames(case, w, h, case.bits, n, True)])
    return gsup, gsf


def _blob_equal(got, want, ad, what):
    if np.array_equal(got, want):
        return
    msg = ["%s: %d bytes differ, first at %d" % (what, int(np.count_nonzero(got != want)), int(np.nonzero(got != want)[0][0]))]
    for level in range(ad.nLvCount):
        (gx, gy, gs), (wx, wy, ws) = pl.blob_vectors(got, ad, level), pl.blob_vectors(want, ad, level)
        d = (gx != wx) | (gy != wy) | (gs != ws)
        if d.any():
            y, x = [int(v[0]) for v in np.nonzero(d)]
            msg.append("level %d: %d of %d records, first (by=%d, bx=%d) got (%d, %d, %d) want (%d, %d, %d)" % (
                level, int(d.sum()), d.size, y, x, gx[y, x], gy[y, x], gs[y, x], wx[y, x], wy[y, x], ws[y, x]))
    pytest.fail("; ".join(msg))


def _planes_equal(mv, got, want, what):
    for p in range(len(want)):
        d = pl.first_diff(mv.plane_to_numpy(got[p], want[p].shape[1], want[p].dtype), want[p])
        if d:
            pytest.fail("%s plane %d: %s" % (what, p, d))


def _consumers(oracle, mv, case, sv, out_ad, gbw, gfw, wbw, wfw):
    """step 2: the scaled blobs (device: gbw, gfw; the restatement's: wbw, wfw) through Degrain1, Compensate and Recalculate at full size"""
    import torch
    _, (tw, th) = sc.sizes(case)
    frames = _frames(case, tw, th, case.tbits, 3, False)
    skw = sc.super_kwargs(case, True)
    osup, gsup = oracle.Super(tw, th, case.tbits, **skw), sv.sup
    osf = [osup.frame(f) for f in frames]
    gsrc = [mv.frame_to_device(f) for f in frames]
    gsf = gsup.build(gsrc)
    # mvbw: frame 1 against frame 2; mvfw: frame 1 against frame 0
    got = mv.Degrain(1, gsup, sv.ad, [p.stride(0) for p in gsrc[1]]).run([(gsrc[1], [gsf[2], gsf[0]], [gbw, gfw])])[0]
    torch.cuda.synchronize()
    _planes_equal(mv, got, oracle.Degrain(1, osup, out_ad).frame(frames[1], [osf[2], osf[0]], [wbw, wfw]), "%s: Degrain1" % case.name)
    got = mv.Compensate(gsup, sv.ad).run([(gsf[1], gsf[2], gbw)])[0]
    torch.cuda.synchronize()
    _planes_equal(mv, got, oracle.Compensate(osup, out_ad).frame(osf[1], osf[2], wbw), "%s: Compensate" % case.name)
    rkw = sc.smaller_blocks(case)
    grc, orc = mv.Recalculate(gsup, sv.ad, **rkw), oracle.Recalculate(osup, out_ad, **rkw)
    assert grc.blob_size == orc.blob_size and grc.ad.nBlkSizeX == case.scale * case.akw["blksize"] // 2
    got = grc.run([(gsf[1], gsf[2], gbw)])[0]
    torch.cuda.synchronize()
    _blob_equal(got.cpu().numpy(), orc.frame(osf[1], osf[2], wbw), orc.ad, "%s: Recalculate %r" % (case.name, rkw))


def _target(mv, case):
    _, (tw, th) = sc.sizes(case)
    return mv.Super(tw, th, case.tbits, **sc.super_kwargs(case, True))


@pytest.mark.parametrize("case", sc.CASES, ids=ids)
def test_scaled_blobs_and_their_consumers(oracle, mv, case):
    import torch
    ssup, ssf = _small(mv, case, 3)
    abw, afw = mv.Analyse(ssup, isb=1, **case.akw), mv.Analyse(ssup, isb=0, **case.akw)
    small = [abw.run([(ssf[1], ssf[2])])[0], afw.run([(ssf[1], ssf[0])])[0]]
    torch.cuda.synchronize()
    edited = [sc.edit_small(case, b.cpu().numpy(), abw.ad, i) for i, b in enumerate(small)]
    dev = [_upload(e, small[0].device) for e in edited]
    sv = mv.ScaleVect(abw.ad, _target(mv, case), case.scale)    # ONE object for both directions: isBackward and nDeltaFrame are labels
    out_ad = ref.scaled_data(abw.ad, case.scale, sv.sup.info)
    assert _fields(sv.ad) == _fields(out_ad) and sv.blob_size == abw.blob_size
    out = sv.run(dev, out=dev) if case.inplace else sv.run(dev)   # both blobs in one launch
    torch.cuda.synchronize()
    want = [ref.scale_blob(e, abw.ad, out_ad, case.scale) for e in edited]
    # step 1, before any consumer sees the blobs
    for i in range(2):
        _blob_equal(out[i].cpu().numpy()[:sv.blob_size], want[i], out_ad, "%s: blob %d against the restatement" % (case.name, i))
        if case.inplace:
            assert out[i].data_ptr() == dev[i].data_ptr()
        else:
            assert np.array_equal(dev[i].cpu().numpy(), edited[i]), "the input blob was written"
        if case.edit == "invalid":
            assert np.array_equal(want[i], edited[i])
        else:
            assert not np.array_equal(want[i], edited[i]) or (case.scale == 1 and case.tbits == case.bits)
    _consumers(oracle, mv, case, sv, out_ad, out[0], out[1], want[0], want[1])


def test_multi_blob_of_radius_two_in_one_call(oracle, mv):
    """every field of a multi blob in one call; the bytes between the fields are neither read into the result nor written"""
    import torch
    case, radius = sc.MULTI, 2
    nr = 2 * radius
    ssup, ssf = _small(mv, case, 2 * radius + 1)
    an = mv.AnalyseN(ssup, radius, **case.akw)
    refs = [ssf[m] if m is not None else None for m in mv.multi_refs(radius, radius, 2 * radius + 1)]
    multi = an.run([(ssf[radius], refs)])[0]
    torch.cuda.synchronize()
    stride, size = an.field_stride, an.field_size
    assert stride > size, "the case needs a gap between the fields"
    host = multi.cpu().numpy().copy()
    for r in range(nr):
        host[r * stride:r * stride + size] = sc.edit_small(case, host[r * stride:r * stride + size], an.ad(r), r)
        host[r * stride + size:(r + 1) * stride] = 0x5A
    sv = mv.ScaleVect(an.ad(0), _target(mv, case), case.scale)
    out_ad = ref.scaled_data(an.ad(0), case.scale, sv.sup.info)
    assert sv.blob_size == size
    gin = _upload(host, multi.device)
    gout = torch.full((nr * stride,), 0xA5, dtype=torch.uint8, device=multi.device)
    sv.run([gin], out=[gout], fields=nr, field_stride=stride)
    torch.cuda.synchronize()
    got, want = gout.cpu().numpy(), ref.scale_multi(host, an.ad(0), out_ad, case.scale, nr, stride)
    assert np.array_equal(gin.cpu().numpy(), host), "the input blob was written"
    for r in range(nr):
        _blob_equal(got[r * stride:r * stride + size], want[r * stride:r * stride + size], out_ad, "field %d against the restatement" % r)
        assert np.all(got[r * stride + size:(r + 1) * stride] == 0xA5), "the gap behind field %d was written" % r
    fields = [gout[r * stride:r * stride + size] for r in range(nr)]
    _consumers(oracle, mv, case, sv, out_ad, fields[0], fields[1], want[:size], want[stride:stride + size])


def test_end_to_end_pan(oracle, mv):
    """a texture that moves by (4, 2) pixels per frame, searched on its 2x2 box mean and scaled by 2: level 0 carries (4 * pel, 2 * pel) on
    every interior block where the oracle's Analyse of the small clip carries (2 * pel, 1 * pel) -- at least 90 % of them, which is a
    condition on the input (tests/test_scale_vect_host.py::test_pan_clip_is_found_by_the_oracle), not a tolerance"""
    import torch
    full, small = sc.pan_clips(256, 160, 2)
    osup, gsup = oracle.Super(128, 80, 8), mv.Super(128, 80, 8)
    oan, gan = oracle.Analyse(osup, isb=1, blksize=8, overlap=4), mv.Analyse(gsup, isb=1, blksize=8, overlap=4)
    osf = [osup.frame(f) for f in small]
    gsf = gsup.build([mv.frame_to_device(f) for f in small])
    ox, oy, _ = pl.blob_vectors(oan.frame(osf[0], osf[1]), oan.ad)
    pel = oan.ad.nPel
    found = (sc.interior(ox) == 2 * pel) & (sc.interior(oy) == 1 * pel)
    assert found.mean() >= 0.9, "the input does not meet its condition: %.3f" % found.mean()
    tsup = mv.Super(256, 160, 8, hpad=32, vpad=32)
    sv = mv.ScaleVect(gan.ad, tsup, 2)
    out = sv.run(gan.run([(gsf[0], gsf[1])]))[0]
    torch.cuda.synchronize()
    x, y, _ = pl.blob_vectors(out.cpu().numpy()[:sv.blob_size], sv.ad)
    assert sv.ad.nPel == pel
    hit = (sc.interior(x) == 4 * pel) & (sc.interior(y) == 2 * pel)
    assert np.all(hit[found]), "%d of %d interior blocks the oracle found do not carry (4 * pel, 2 * pel)" % (int(np.count_nonzero(found & ~hit)), int(found.sum()))
