"""GPU: RecalculateN through the Python package (the C ABI beneath it), byte for byte against the CPU oracle.

The old multi blobs are searched by AnalyseN on the device (held to the oracle's fields here as well, so that a difference names its stage), every
frame of the clip is a job of ONE RecalculateN call -- both clip ends, with references outside the clip, are in every case -- and every field of
every frame is compared with oracle.Recalculate on the oracle's field.  The blobs are written over a sentinel: the pad bytes between fields must
still carry it.  tests/test_multi_recalculate_cases.py shows on the CPU that at the cases' thsad some blocks are searched again and some are not."""
import numpy as np
import pytest

import degrain_n_cases as dc
import multi_oracle as mu
import pipeline as pl

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_dev = {}


class Dev:
    """the clip of an oracle-side Multi on the device: super frames, reference tables, the multi blob of every frame from ONE AnalyseN call"""

    def __init__(self, mv, m):
        import torch
        self.m = m
        self.sup = mv.Super(m.w, m.h, m.bits, **dict(dc.FORMATS[m.fmt], **m.skw))
        self.src = [mv.frame_to_device(f) for f in m.frames]
        self.sf = self.sup.build(self.src)
        self.an = mv.AnalyseN(self.sup, m.radius, num_frames=m.n, **m.akw)
        self.refs = [[self.sf[k] if k is not None else None for k in mv.multi_refs(n, m.radius, m.n)] for n in range(m.n)]
        self.multi = self.an.run([(self.sf[n], self.refs[n]) for n in range(m.n)])
        torch.cuda.synchronize()


def _device(mv, m):
    if id(m) not in _dev:
        _dev[id(m)] = Dev(mv, m)
    return _dev[id(m)]


def _recalculated(mv, case):
    import torch
    m = mu.recalc_multi(case)
    d = _device(mv, m)
    rn = mv.RecalculateN(d.sup, d.an.ad(0), m.radius, **mu.recalc_kwargs(case))
    out = rn.alloc_blobs(m.n)
    for b in out:
        b.fill_(SENTINEL)
    got = rn.run([(d.sf[n], d.refs[n], d.multi[n]) for n in range(m.n)], blobs=out)
    torch.cuda.synchronize()
    return m, d, rn, got


@pytest.mark.parametrize("case", mu.recalc_cases(), ids=mu.recalc_id)
def test_every_field_is_oracle_recalculate_on_the_oracles_field(mv, case):
    m, d, rn, got = _recalculated(mv, case)
    ads, want = m.recalc(**mu.recalc_kwargs(case))
    size, stride = rn.field_size, rn.field_stride
    assert 0 < size < stride and got[0].numel() == rn.blob_size == 2 * m.radius * stride
    invalid = changed = 0
    for n in range(m.n):
        old = d.multi[n].cpu().numpy()
        whole = got[n].cpu().numpy()
        for r in range(2 * m.radius):
            o = old[r * d.an.field_stride:r * d.an.field_stride + d.an.field_size]
            assert np.array_equal(o, m.blobs[n][r]), "AnalyseN: frame %d field %d" % (n, r)
            assert want[n][r].size == size
            assert np.array_equal(whole[r * stride:r * stride + size], want[n][r]), "frame %d field %d: %s" % (n, r, pl.first_diff(whole[r * stride:r * stride + size], want[n][r]))
            assert (whole[r * stride + size:(r + 1) * stride] == SENTINEL).all(), "pad bytes behind field %d of frame %d" % (r, n)
            valid = int(want[n][r][4:8].view(np.int32)[0])
            assert valid == (m.nref(n, r) is not None)
            invalid += not valid
        changed += not np.array_equal(rn.fields(got[n])[0].cpu().numpy()[:64], old[:64])
    assert invalid == m.radius * (m.radius + 1)  # (each clip end: radius + (radius - 1) + ... + 1 references outside the clip)
    for r in range(2 * m.radius):
        assert bytes(rn.get_data(r)) == bytes(ads[r]), "field %d" % r
    assert changed  # (another geometry: not the old blob handed through)


def test_jobs_in_one_call_are_the_jobs_run_singly(mv):
    import torch
    case = ("420", 8, mu.R168_84, 3, {})
    m, d, rn, together = _recalculated(mv, case)
    for n in (0, 4, m.n - 1):
        alone = rn.run([(d.sf[n], d.refs[n], d.multi[n])])[0]
        torch.cuda.synchronize()
        for r, (a, b) in enumerate(zip(rn.fields(alone), rn.fields(together[n]))):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), (n, r)


def test_recalculated_blobs_feed_degrain_n(mv, oracle):
    """RecalculateN.run -> DegrainN.run on the multi blob, against oracle.Degrain on the oracle's recalculated fields"""
    import torch
    case = ("420", 8, mu.R168_84, 3, {})
    m, d, rn, got = _recalculated(mv, case)
    ads, blobs = m.recalc(**mu.recalc_kwargs(case))
    pitch = [p.stride(0) for p in d.src[0]]
    dg = mv.DegrainN(m.radius, d.sup, rn.get_data(0), pitch)
    frames = [m.radius + 1, 0, m.n - 1]
    out = dg.run([(d.src[n], d.refs[n], got[n]) for n in frames])
    torch.cuda.synchronize()
    ref = oracle.Degrain(m.radius, m.osup, ads[0])
    for j, n in enumerate(frames):
        want = ref.frame(m.frames[n], [m.ref(n, r) for r in range(2 * m.radius)], blobs[n])
        for p in range(3):
            g = mv.plane_to_numpy(out[j][p], want[p].shape[1], want[p].dtype)
            assert pl.first_diff(g, want[p]) == "", "frame %d plane %d" % (n, p)
        assert not np.array_equal(want[0], m.frames[n][0])
