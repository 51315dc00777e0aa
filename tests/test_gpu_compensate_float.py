"""GPU: Compensate and CompensateN on a float clip (mvx_compensate_create_float, mvx_compensate_n_create_float) against the numpy restatement
(tests/compensate_float_ref.py, anchored to the oracle by tests/test_compensate_float_ref.py), sample for sample: np.array_equal on float32 and no
NaN in any result.

The rig is that of tests/test_gpu_degrain_float.py: the float clip is float_clip of the integer clip, the vectors are searched by AnalyseN on the
integer copy, never on the float samples, and the float super frames are built on the GPU and asserted to be the Super restatement's
(tests/super_float_ref.py) before the restatement runs on them.  Every frame of the clip is a job, so both clip ends -- references outside the
clip -- are in every searched case.  tests/test_compensate_float_cases.py shows on the CPU that at the cases' thsad most far blocks are compensated
and some are not; the same is asserted here from the searched fields."""
import numpy as np
import pytest

import compensate_float_cases as cc
import compensate_float_ref as cf
import degrain_float_cases as fc
import degrain_n_cases as dc
import layouts as lo
import multi_cases as mc
import pipeline as pl
import super_float_ref as sf
import vector_fields

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 3
SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "gray": (1, 1)}
_clips = {}


class Clip:
    """the integer clip with its super frames and the multi blob of every frame (ONE AnalyseN call), and the float clip with its float super
    frames, on the device"""

    def __init__(self, mv, fmt, bits, blk, tr, w, h):
        import torch
        self.mv, self.fmt, self.tr, self.w, self.h = mv, fmt, tr, w, h
        self.q = dc.clip(w, h, bits, mc.nframes(tr), fmt)
        self.frames = fc.float_clip(self.q, bits, seed=9)
        self.n = len(self.q)
        kw = dict(dc.FORMATS[fmt], **blk[1])
        self.isup = mv.Super(w, h, bits, **kw)
        self.isf = self.isup.build([mv.frame_to_device(f) for f in self.q])
        self.an = mv.AnalyseN(self.isup, tr, num_frames=self.n, **blk[2])
        self.nrefs = [mv.multi_refs(n, tr, self.n) for n in range(self.n)]
        self.multi = self.an.run([(self.isf[n], [self.isf[m] if m is not None else None for m in self.nrefs[n]]) for n in range(self.n)])
        self.fsup = mv.Super(w, h, 32, sample_float=True, **kw)
        self.fsf = self.fsup.build([mv.frame_to_device(f) for f in self.frames])
        self.refs = [[self.fsf[m] if m is not None else None for m in row] for row in self.nrefs]
        i = self.fsup.info
        self.skw = dict(sub=SUB[fmt], gray=fmt == "gray", hpad=i.hpad, vpad=i.vpad, pel=i.pel, sharp=i.sharp)
        torch.cuda.synchronize()
        self.host_fields = [[np.asarray(f.cpu().numpy()) for f in self.an.fields(self.multi[n])] for n in range(self.n)]
        self.host = {}

    def sup_np(self, m):
        """the GPU-built float super frame m on the host; asserted to be the Super restatement's when first fetched"""
        if m is None:
            return None
        if m not in self.host:
            got = [self.mv.plane_to_numpy(self.fsf[m][p], self.fsup.info.plane_width[p], np.float32) for p in range(self.fsup.nplanes)]
            want, _ = sf.frame(self.frames[m], **self.skw)
            for p in range(self.fsup.nplanes):
                assert np.array_equal(got[p], want[p]), "float Super differs from its restatement: frame %d plane %d" % (m, p)
            self.host[m] = got
        return self.host[m]

    def planes(self, frame):
        return [_np(self.mv, frame[p], self.frames[0][p].shape[1]) for p in range(len(self.frames[0]))]


def _np(mv, t, width):
    import torch
    return mv.plane_to_numpy(t if t.dtype == torch.uint8 else t.view(torch.uint8), width, np.float32)


def _clip(mv, fmt, bits, blk, tr, w=mc.W, h=mc.H):
    key = (fmt, bits, blk[0], tr, w, h)
    if key not in _clips:
        _clips[key] = Clip(mv, fmt, bits, blk, tr, w, h)
    return _clips[key]


def _guarded(c, count):
    """count float frames whose planes lie inside sentinel-filled buffers: GUARD rows above and below, the pitch padding to the right"""
    import torch
    hs, ws = [p.shape[0] for p in c.frames[0]], [p.shape[1] for p in c.frames[0]]
    pitch = [(w * 4 + 255) // 256 * 256 for w in ws]
    bufs = [[torch.full((hs[p] + 2 * GUARD, pitch[p]), SENTINEL, dtype=torch.uint8, device="cuda") for p in range(len(ws))] for _ in range(count)]
    views = [[b[p][GUARD:GUARD + hs[p]] for p in range(len(ws))] for b in bufs]
    return bufs, views, [w * 4 for w in ws], pitch


def _guard_intact(bufs, rowbytes):
    for fr in bufs:
        for p, b in enumerate(fr):
            a = b.cpu().numpy()
            if not ((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all() and (a[:, rowbytes[p]:] == SENTINEL).all()):
                return False
    return True


def _run_n(mv, c, ckw, frames=None, multi=None):
    """CompensateN(sample_float=True) over `frames` of the clip (all by default) in one call into guarded planes -> {(n, k): planes}"""
    import torch
    frames = list(range(c.n)) if frames is None else frames
    multi = multi or c.multi
    cn = mv.CompensateN(c.tr, c.fsup, c.an.ad(0), sample_float=True, **ckw)
    no = 2 * c.tr + 1
    bufs, views, rowbytes, pitch = _guarded(c, no * len(frames))
    assert cn.is_float and cn.dst_pitch == pitch
    out = [views[j * no:(j + 1) * no] for j in range(len(frames))]
    cn.run([(c.fsf[n], c.refs[n], multi[n]) for n in frames], out=out)
    torch.cuda.synchronize()
    assert _guard_intact(bufs, rowbytes), "a destination plane's guard band was written"
    return {(n, k): c.planes(out[j][k]) for j, n in enumerate(frames) for k in range(no)}


def _want_n(oracle, c, ckw, n, blobs=None):
    ref = cc.restatement(oracle, c.an.ad(0), ckw, gray=c.fmt == "gray")
    return ref.job(c.tr, c.sup_np(n), [c.sup_np(m) for m in c.nrefs[n]], blobs or c.host_fields[n])


def _same(got, want, what):
    assert len(got) == len(want)
    for p in range(len(want)):
        assert got[p].dtype == np.float32 and want[p].dtype == np.float32 and not np.isnan(got[p]).any(), "%s plane %d" % (what, p)
        assert pl.first_diff(got[p], want[p]) == "", "%s plane %d: %s" % (what, p, pl.first_diff(got[p], want[p]))


def _bits(planes):
    return [np.ascontiguousarray(p).view(np.uint32) for p in planes]


def _check_all(oracle, c, ckw, got, frames, blobs=None):
    """every output of every job against the restatement; the centre bit for bit the clip frame -> the number of outputs that are not the source"""
    moved = 0
    for n in frames:
        want = _want_n(oracle, c, ckw, n, blobs[n] if blobs else None)
        for k in range(2 * c.tr + 1):
            _same(got[(n, k)], want[k], "frame %d output %d" % (n, k))
            if k == c.tr:
                assert all(np.array_equal(a, b) for a, b in zip(_bits(got[(n, k)]), _bits(c.frames[n]))), "the centre of frame %d" % n
            elif 0 <= n + k - c.tr < c.n:
                moved += not np.array_equal(got[(n, k)][0], c.frames[n][0])
    return moved


# ------------------------------------------------------------------------------------------------ searched vectors, every frame a job

@pytest.mark.parametrize("case", cc.SEARCHED, ids=cc.case_id)
def test_every_output_of_every_job_is_the_restatements(oracle, mv, case):
    fmt, bits, blk, tr, w, h, thsad = case
    c = _clip(mv, fmt, bits, blk, tr, w, h)
    sads = [pl.blob_vectors(f, c.an.ad(r))[2] for r, f in enumerate(c.host_fields[tr + 1])]
    used, unused = mc.far_shares(sads, c.an.ad(0), thsad, tr)
    assert used >= mc.USED and unused >= mc.UNUSED
    ckw = dict(thsad=thsad)
    moved = _check_all(oracle, c, ckw, _run_n(mv, c, ckw), range(c.n))
    assert moved >= tr  # (compensated frames are not copies of the source)


@pytest.mark.parametrize("blk,bits", [(mc.B84, 16), (mc.B160, 8)], ids=["8/4", "16/0"])
def test_time_50(oracle, mv, blk, bits):
    c = _clip(mv, "420", bits, blk, 3 if blk is mc.B84 else 7)
    n = c.tr + 1
    full = _run_n(mv, c, dict(thsad=mc.THSAD), frames=[n])
    ckw = dict(thsad=mc.THSAD, time=50.0)
    half = _run_n(mv, c, ckw, frames=[n, 0])
    _check_all(oracle, c, ckw, half, [n, 0])
    assert any(not np.array_equal(full[(n, k)][0], half[(n, k)][0]) for k in range(2 * c.tr + 1))


@pytest.mark.parametrize("scbehavior", [0, 1])
@pytest.mark.parametrize("bits,blk", [(16, mc.B84), (16, mc.B160)], ids=["8/4", "16/0"])
def test_a_scene_change_in_one_field(oracle, mv, bits, blk, scbehavior):
    """field 3 (forward, distance 2) of the middle frame carries one block too many above thscd1 (tests/vector_fields.py scene_count): that
    output is the reference frame at scbehavior 0 and the source at 1, bit for bit, and the other outputs are not touched by it"""
    import torch
    tr, n, field = 3, 4, 3
    c = _clip(mv, "420", bits, blk, tr)
    ad = c.an.ad(field)
    th, s1, s2 = vector_fields.scaled_thresholds(ad, mc.THSAD)
    multi = list(c.multi)
    multi[n] = c.multi[n].clone()
    view = c.an.fields(multi[n])[field]
    edited = vector_fields.scene_count(view.cpu().numpy(), ad, 77, s1, s2 + 1, th)
    view.copy_(torch.from_numpy(edited).to(view.device))
    blobs = {m: list(c.host_fields[m]) for m in (n, 0)}
    blobs[n][field] = edited
    ckw = dict(thsad=mc.THSAD, scbehavior=scbehavior)
    got = _run_n(mv, c, ckw, frames=[n, 0], multi=multi)
    _check_all(oracle, c, ckw, got, [n, 0], blobs)
    k = tr - 2
    want = c.frames[n] if scbehavior else c.frames[n - 2]
    assert all(np.array_equal(a, b) for a, b in zip(_bits(got[(n, k)]), _bits(want)))
    assert not np.array_equal(got[(n, k)][0], _run_n(mv, c, ckw, frames=[n])[(n, k)][0])  # (without the edit that output is a compensated frame)


# ------------------------------------------------------------------------------------------------ crafted fields on the small sizes

SMALL = [("420", 16, mc.B84, 2, 70, 54), ("420", 16, mc.B160, 2, 70, 54), ("420", 8, cc.B42P1, 1, 70, 54), ("gray", 16, cc.B84P0, 2, 36, 36)]


@pytest.mark.parametrize("fmt,bits,blk,tr,w,h", SMALL, ids=["70x54-8/4", "70x54-16/0", "70x54-4/2-pel1", "36x36-gray-pad0"])
def test_vectors_on_the_limits_of_their_legal_rectangles_and_an_invalid_blob(oracle, mv, fmt, bits, blk, tr, w, h):
    """every field of the middle frame and of the first: a quarter of the blocks on each end of the legal rectangle in each component, a tenth
    of them falling back on the source (compensate_float_cases.with_fallbacks) -- the float super frames are read up to the far edges of their
    padding, in every sub-pel plane; one field of the middle frame is an invalid blob; the destinations lie inside guard bands"""
    import torch
    c = _clip(mv, fmt, bits, blk, tr, w, h)
    n, dead = tr + 1, 1
    multi, blobs = list(c.multi), {}
    for m in (n, 0):
        multi[m] = c.multi[m].clone()
        blobs[m] = []
        for r, view in enumerate(c.an.fields(multi[m])):
            b = cc.with_fallbacks(c.host_fields[m][r], c.an.ad(r), 300 + 10 * m + r, 300)
            if m == n and r == dead:
                b = vector_fields.invalid(b, c.an.ad(r))
            view.copy_(torch.from_numpy(b).to(view.device))
            blobs[m].append(b)
    xmin, xmax, ymin, ymax = vector_fields.legal_rect(c.an.ad(0))
    on = np.zeros(4, bool)  # over the live fields of the middle frame (a grid of 4 x 3 blocks need not reach every limit in one field)
    for r in range(2 * tr):
        if r != dead:
            vx, vy, _ = pl.blob_vectors(blobs[n][r], c.an.ad(r))
            on |= [(vx == xmin[None, :]).any(), (vx == xmax[None, :]).any(), (vy == ymin[:, None]).any(), (vy == ymax[:, None]).any()]
    assert on.all(), on
    for scb in (0, 1):
        ckw = dict(thsad=300, scbehavior=scb)
        got = _run_n(mv, c, ckw, frames=[n, 0], multi=multi)
        _check_all(oracle, c, ckw, got, [n, 0], blobs)
        k = [k for k in range(2 * tr + 1) if cf.field_of(tr, k) == dead][0]
        want = c.frames[n] if scb else c.frames[c.nrefs[n][dead]]
        assert all(np.array_equal(a, b) for a, b in zip(_bits(got[(n, k)]), _bits(want))), "the invalid field at scbehavior %d" % scb


LAYOUTS = [("tight", "sup16"), ("plus1", "sup256"), ("offset", "sup16"), ("padded", None)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "%s-%s" % (l[0], l[1] or "sup"))
@pytest.mark.parametrize("fmt,bits,blk,tr,w,h", [SMALL[0], SMALL[2], SMALL[3]], ids=["70x54-8/4", "70x54-4/2-pel1", "36x36-gray-pad0"])
def test_planes_carved_out_of_arenas_of_quiet_nans(oracle, mv, fmt, bits, blk, tr, w, h, layout):
    """super frames built by the GPU into arenas filled with quiet NaNs (and with the two byte fills), destinations carved out of such arenas at
    tight, odd-pitch and offset layouts: no stray read reaches a result, nothing but samples is written, no input changes"""
    import test_gpu_layouts as tl
    c = _clip(mv, fmt, bits, blk, tr, w, h)
    n = tr + 1
    ckw = dict(thsad=300)
    want = _want_n(oracle, c, ckw, n)
    kw = dict(dc.FORMATS[fmt], **blk[1])
    for fill in (lo.NAN_FILL,) + tuple(lo.FILLS):
        rig = tl.Rig(mv, c.frames, w, h, 32, dict(sample_float=True, **kw), fill, "padded", layout[1])
        outs = [rig.clip_frame(layout[0], shapes=[a.shape for a in c.frames[n]]) for _ in range(2 * tr + 1)]
        cn = mv.CompensateN(tr, rig.sup, c.an.ad(0), [v.stride(0) for v in outs[0][0]], sample_float=True, **ckw)
        rig.freeze()
        cn.run([(rig.sf[n], [rig.sf[m] if m is not None else None for m in c.nrefs[n]], c.multi[n])], out=[[o[0] for o in outs]])
        rig.sync()
        name = "NaN fill" if not isinstance(fill, int) else "fill 0x%02x" % fill
        for k, (views, guards) in enumerate(outs):
            _same([lo.get(views[p], want[k][p].shape[1], np.float32) for p in range(len(want[k]))], want[k], "%s output %d" % (name, k))
            for p, g in enumerate(guards):
                damage = lo.intact(*g[:3], g[3])
                assert not damage, "%s output %d plane %d: %s" % (name, k, p, lo.describe(damage))
        assert all(bool((a == s_).all()) for (_, a), s_ in zip(rig.inputs, rig.snap)), "%s: an input was written" % name


# ------------------------------------------------------------------------------------------------ against the oracle directly

@pytest.mark.parametrize("bits,pel,akw,ckw", [(8, 1, dict(blksize=16, overlap=0), dict(thsad=250)), (16, 2, dict(blksize=8, overlap=0), dict(thsad=250, time=50.0)),
                                              (8, 2, dict(blksize=8, overlap=4), dict(thsad=250)), (16, 2, dict(blksize=16, overlap=8), {}),
                                              (16, 1, dict(blksize=4, overlap=2), dict(thsad=250, scbehavior=0))],
                         ids=["8bit-pel1-16/0", "16bit-pel2-8/0-time50", "8bit-pel2-8/4", "16bit-pel2-16/8", "16bit-pel1-4/2"])
def test_integer_valued_super_frames_against_the_oracle(oracle, mv, bits, pel, akw, ckw):
    """the oracle's level-0 super rows uploaded as an integer-valued float super frame, its blobs uploaded: with overlap 0 the outputs are
    oracle.Compensate's samples exactly; with overlap they stay within the bound tests/test_compensate_float_ref.py derives"""
    import torch
    w, h, n = 104, 70, 3  # strips right and below
    frames = dc.clip(w, h, bits, n)
    osup = oracle.Super(w, h, bits, pel=pel)
    osf = [osup.frame(f) for f in frames]
    fsup = mv.Super(w, h, 32, sample_float=True, pel=pel)
    one = oracle.Super(w, h, bits, pel=pel, levels=1)  # level 0 opens every plane of the oracle's super frame
    assert [one.plane_shape(p) for p in range(3)] == [(fsup.info.plane_height[p], fsup.info.plane_width[p]) for p in range(3)]
    fsf = [fsup.from_host([p[:fsup.info.plane_height[i]].astype(np.float32) for i, p in enumerate(fr)]) for fr in osf]
    bound = 0.0 if not akw["overlap"] else cc.bound((1 << bits) - 1)
    worst = 0.0
    for isb, delta, m, r in ((1, 1, 1, 2), (0, 1, 1, 0), (1, 2, 0, 2)):
        oan = oracle.Analyse(osup, num_frames=n, isb=isb, delta=delta, **akw)
        blob = oan.frame(osf[m], osf[r])
        want = oracle.Compensate(osup, oan.ad, **ckw).frame(osf[m], osf[r], blob)
        comp = mv.Compensate(fsup, oan.ad, sample_float=True, **ckw)
        out = comp.run([(fsf[m], fsf[r], torch.from_numpy(blob).to("cuda"))])[0]
        torch.cuda.synchronize()
        assert all(o.dtype == torch.float32 for o in out)
        for p in range(3):
            got = _np(mv, out[p], want[p].shape[1])
            assert not np.isnan(got).any()
            err = float(np.abs(got.astype(np.float64) - want[p].astype(np.float64)).max())
            worst = max(worst, err)
            assert err <= bound, "isb %d delta %d plane %d: %.4f > %.4f" % (isb, delta, p, err, bound)
        assert not np.array_equal(want[0], frames[m][0])
    print("max |float - oracle| = %.4f (bound %.4f)" % (worst, bound))


# ------------------------------------------------------------------------------------------------ the single form against CompensateN

@pytest.mark.parametrize("blk", [mc.B84, mc.B160], ids=["8/4", "16/0"])
def test_single_compensate_is_bit_for_bit_compensate_n(mv, blk):
    """Compensate(sample_float=True) on (source, reference, field) for backward and forward fields of distance 1, 2 and 3, every frame of the
    clip, both ends included: the bits of CompensateN's output for that field"""
    import torch
    c = _clip(mv, "420", 16, blk, 3)
    ckw = dict(thsad=mc.THSAD)
    many = _run_n(mv, c, ckw)
    cn = mv.CompensateN(3, c.fsup, c.an.ad(0), sample_float=True, **ckw)
    seen = []
    for k in range(7):
        off, field = cn.map(k)
        if field < 0:
            continue
        ad = c.an.ad(field)
        seen.append((bool(ad.isBackward), ad.nDeltaFrame))
        comp = mv.Compensate(c.fsup, ad, sample_float=True, **ckw)
        assert comp.is_float
        outs = comp.run([(c.fsf[n], c.refs[n][field], c.an.fields(c.multi[n])[field]) for n in range(c.n)])
        torch.cuda.synchronize()
        for n in range(c.n):
            assert all(o.dtype == torch.float32 for o in outs[n])
            for a, b in zip(_bits(c.planes(outs[n])), _bits(many[(n, k)])):
                assert np.array_equal(a, b), "frame %d output %d" % (n, k)
    assert (False, 2) in seen and (True, 2) in seen and (False, 1) in seen and len(seen) == 6


def test_jobs_in_one_call_are_the_jobs_run_singly(mv):
    c = _clip(mv, "420", 16, mc.B84, 3)
    together = _run_n(mv, c, dict(thsad=mc.THSAD), frames=[4, 0, 8, 5])
    for n in (4, 0, 8, 5):
        alone = _run_n(mv, c, dict(thsad=mc.THSAD), frames=[n])
        for k in range(7):
            assert all(np.array_equal(a, b) for a, b in zip(_bits(together[(n, k)]), _bits(alone[(n, k)]))), (n, k)


# ------------------------------------------------------------------------------------------------ the package, end to end

def test_torch_float32_planes_end_to_end(oracle, mv):
    """Super(sample_float=True).build -> AnalyseN on the integer copy -> CompensateN(sample_float=True) -> DegrainN on plain torch.float32 planes
    (rows of width samples, no padding): CompensateN allocates float32 planes by the float pitch, and both filters are their restatements"""
    import torch
    w, h, n, tr = 72, 56, 5, 2
    q = dc.clip(w, h, 16, n)
    frames = fc.float_clip(q, 16, seed=4)
    isup = mv.Super(w, h, 16)
    isf = isup.build([mv.frame_to_device(f) for f in q])
    an = mv.AnalyseN(isup, tr, num_frames=n, **dict(blksize=8, overlap=4))
    nrefs = mv.multi_refs(2, tr, n)
    mb = an.run([(isf[2], [isf[m] for m in nrefs])])[0]
    src = [[torch.from_numpy(p).to("cuda") for p in f] for f in frames]
    assert src[0][0].dtype == torch.float32 and src[0][0].stride(0) == w
    fsup = mv.Super(w, h, bits=32, sample_float=True)
    fsf = fsup.build(src)
    cn = mv.CompensateN(tr, fsup, an.ad(0), sample_float=True, thsad=300)
    assert cn.dst_pitch == [512, 256, 256]
    out = cn.run([(fsf[2], [fsf[m] for m in nrefs], mb)])[0]
    tight = mv.CompensateN(tr, fsup, an.ad(0), [w * 4, w * 2, w * 2], sample_float=True, thsad=300)
    out_tight = [[torch.empty_like(p) for p in src[2]] for _ in range(2 * tr + 1)]
    tight.run([(fsf[2], [fsf[m] for m in nrefs], mb)], out=[out_tight])
    dg = mv.DegrainN(tr, fsup, an.ad(0), [w * 4, w * 2, w * 2])
    den = dg.run([(src[2], [fsf[m] for m in nrefs], mb)])[0]
    torch.cuda.synchronize()
    assert len(out) == 2 * tr + 1 and all(o.dtype == torch.float32 and o.shape == (s.shape[0], 512 // 4 if p == 0 else 256 // 4)
                                          for fr in out for p, (o, s) in enumerate(zip(fr, src[2])))
    sup_np = {m: [mv.plane_to_numpy(fsf[m][p], fsup.info.plane_width[p], np.float32) for p in range(3)] for m in range(n)}
    for m in range(n):
        want, _ = sf.frame(frames[m])
        assert all(np.array_equal(sup_np[m][p], want[p]) for p in range(3))
    blobs = [np.asarray(f.cpu().numpy()) for f in an.fields(mb)]
    want = cc.restatement(oracle, an.ad(0), dict(thsad=300)).job(tr, sup_np[2], [sup_np[m] for m in nrefs], blobs)
    for k in range(2 * tr + 1):
        _same([o[:, :s.shape[1]].cpu().numpy() for o, s in zip(out[k], src[2])], want[k], "output %d" % k)
        _same([o.cpu().numpy() for o in out_tight[k]], want[k], "tight output %d" % k)
    assert all(torch.equal(a, b) for a, b in zip(out_tight[tr], src[2]))                          # the centre is the clip frame
    ref = fc.restatement(oracle, tr, an.ad(0), dg.info()["thsad_d"], dg.info()["thsadc_d"], {})
    _same([o.cpu().numpy() for o in den], ref.frame(frames[2], [sup_np[m] for m in nrefs], blobs), "DegrainN")
    with pytest.raises(mv.MvtoolsError, match="CompensateN: float super clips are not supported."):
        mv.CompensateN(tr, fsup, an.ad(0))
