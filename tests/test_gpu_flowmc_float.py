"""GPU: Flow and FlowBlur on float clips (mvx_flowcomp_create_float, mvx_flowblur_create_float) against the numpy restatement
(tests/flowmc_float_ref.py, anchored to the integer restatement by tests/test_flowmc_float_ref.py), bit for bit: planes are compared as uint32, so
NaN payloads and signed zeros count.

The rig is that of the other float filters: the float clip is float_clip of the integer clip, the vectors are searched on the integer copy and
never on the float samples, crafted cases rewrite them on the host, and the float super frames are built on the GPU and asserted to be the Super
restatement's (tests/super_float_ref.py) before the restatement runs on them.  The search is mv.Analyse's on the GPU at every size, the two tiny clips
(36x36 without padding, 35x30) included: the unpadded 36x36 search once ended in a memory fault, tests/test_gpu_small_geometry.py has what
it was.  Every frame of a case's clip is a job of ONE call, so copied
frames (clip ends, scene changes, invalid blobs) stand beside compensated ones in every batch; tests/test_flowmc_float_cases.py holds the cases
to their conditions on the CPU, and the same conditions are asserted here from the vectors the GPU searched."""
import numpy as np
import pytest

import flowmc_float_cases as fx
import flowmc_float_ref as ff
import layouts as lo
import super_float_ref as sf
from test_gpu_parity import dbg  # noqa: F401  (the fixture that puts a debug option back)

pytestmark = pytest.mark.gpu

F = np.float32
HOST_SEARCH = ()  # (sizes searched by the oracle on the host instead: none -- the fault of the unpadded 36x36 search is fixed, tests/test_gpu_small_geometry.py)
_rigs = {}


class Rig:
    """one case on the device: the integer clip's super frames and searched blobs (edited on the host by the case's recipes), the float clip
    and its float super frames, and the restatement's frames for them"""

    def __init__(self, mv, oracle, c):
        import torch
        self.mv, self.c = mv, c
        self.q, self.floats = fx.clips(c)
        kw = fx.super_kwargs(c)
        searched = fx.search_oracle(oracle, c, self.q) if (c.w, c.h) in HOST_SEARCH else []
        if not searched:
            isup = mv.Super(c.w, c.h, c.bits, **kw)
            isf = isup.build([mv.frame_to_device(f) for f in self.q])
        for isb, delta in [] if searched else fx.fields(c):
            an = mv.Analyse(isup, num_frames=fx.NF, isb=isb, delta=delta, **fx.analyse_kwargs(c))
            refs = [fx.reference(isb, delta, n) for n in range(fx.NF)]
            blobs = an.run([(isf[n], isf[r] if r is not None else None) for n, r in enumerate(refs)])
            torch.cuda.synchronize()
            searched.append((an.ad, [b.cpu().numpy() for b in blobs]))
        self.vectors = fx.edited(c, searched)
        self.blobs = [[torch.from_numpy(b).to("cuda") for b in blobs] for _, blobs in self.vectors]
        self.fsup = mv.Super(c.w, c.h, 32, sample_float=True, **kw)
        self.src = [mv.frame_to_device(f) for f in self.floats]
        self.fsf = self.fsup.build(self.src)
        self.pitch = [p.stride(0) for p in self.src[0]]
        torch.cuda.synchronize()
        i = self.fsup.info
        skw = dict(sub=fx.SUB[c.fmt], gray=c.fmt == "gray", hpad=i.hpad, vpad=i.vpad, pel=i.pel, sharp=i.sharp)

        def sup(k):  # the GPU-built float super frame k on the host, asserted to be the Super restatement's
            got = [mv.plane_to_numpy(self.fsf[k][p], i.plane_width[p], F) for p in range(self.fsup.nplanes)]
            want, _ = sf.frame(self.floats[k], **skw)
            for p in range(self.fsup.nplanes):
                assert np.array_equal(got[p], want[p]), "float Super differs from its restatement: frame %d plane %d" % (k, p)
            return got
        self.want = fx.Expected(c, self.floats, self.vectors, i, supers=sup)

    def make(self, clip_pitch=None, dst_pitch=None):
        mv, c = self.mv, self.c
        if c.kind == "flow":
            return mv.Flow(self.fsup, self.vectors[0][0], fx.NF, clip_pitch or self.pitch, dst_pitch=dst_pitch, sample_float=True, **c.fkw)
        return mv.FlowBlur(self.fsup, self.vectors[0][0], self.vectors[1][0], fx.NF, clip_pitch or self.pitch, dst_pitch=dst_pitch, sample_float=True, **c.fkw)

    def run(self, g, ns, src=None, out=None):
        """frames ns as the jobs of one call of handle g -> the output frames (device planes)"""
        src = src or self.src
        if self.c.kind == "flow":
            inside = lambda k: 0 <= k < fx.NF
            return g.run([(src[n], self.fsf[g.ref(n)] if inside(g.ref(n)) else None, self.blobs[0][n]) for n in ns], out=out)
        return g.run(list(ns), src, self.fsf, self.blobs[0], self.blobs[1], out=out)


def _rig(mv, oracle, c):
    if fx.case_id(c) not in _rigs:
        _rigs[fx.case_id(c)] = Rig(mv, oracle, c)
    return _rigs[fx.case_id(c)]


def _case(cases, name):
    return [c for c in cases if c.name == name][0]


def _np(mv, t, width):
    import torch
    return mv.plane_to_numpy(t if t.dtype == torch.uint8 else t.view(torch.uint8), width, F)


def _same(mv, got, want, what):
    """device planes against host planes, bit for bit"""
    assert len(got) == len(want)
    for p in range(len(want)):
        a, b = ff.bits(_np(mv, got[p], want[p].shape[1])), ff.bits(want[p])
        if not np.array_equal(a, b):
            y, x = [int(v[0]) for v in np.nonzero(a != b)]
            raise AssertionError("%s plane %d: %d samples differ, first at (%d, %d): 0x%08x, wanted 0x%08x" % (what, p, int((a != b).sum()), y, x, a[y, x], b[y, x]))


# ------------------------------------------------------------------------------------------------ every case, every frame a job of one call

@pytest.mark.parametrize("c", fx.CASES, ids=fx.case_id)
def test_every_frame_of_a_case_is_the_restatements(oracle, mv, c):
    import torch
    r = _rig(mv, oracle, c)
    fx.check_conditions(c, r.want)
    g = r.make()
    assert g.is_float
    out = r.run(g, range(fx.NF))
    torch.cuda.synchronize()
    for n in range(fx.NF):
        assert all(o.dtype == torch.float32 for o in out[n])
        _same(mv, out[n], r.want.frames[n], "frame %d (%s)" % (n, r.want.kinds[n]))
        if r.want.kinds[n] == "copy":
            _same(mv, out[n], r.floats[n], "the copied frame %d" % n)


def test_the_searched_shift_cases_have_holes_and_contested_destinations_between_them(oracle, mv):
    stats = [_rig(mv, oracle, c).want.stats for c in fx.FLOW_SEARCHED if c.fkw.get("mode")]
    assert sum(s.get("hole", 0) for s in stats) >= 1 and sum(s.get("collide", 0) for s in stats) >= 1


# ------------------------------------------------------------------------------------------------ copies move bits

ODD = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x7F7FFFFF], np.uint32)
THREE = [(fx.FLOW_SEARCHED, "70x54-8bit-pel2-4/2-fw"), (fx.FLOW_SEARCHED, "70x54-16bit-pel2-4/2-bw-shift"), (fx.BLUR_CRAFTED, "70x54-limits-blur50")]


@pytest.mark.parametrize("cases,name", THREE, ids=["fetch", "shift", "blur"])
def test_a_copied_frame_keeps_quiet_nans_with_their_payloads(oracle, mv, cases, name):
    """the clip frames of the copying jobs are filled with quiet NaNs of several payloads, negative zero, infinities, a denormal: the output is
    those bits, and the compensated frame beside them is untouched by it"""
    import torch
    r = _rig(mv, oracle, _case(cases, name))
    copies = [n for n in range(fx.NF) if r.want.kinds[n] == "copy"]
    usable = [n for n in range(fx.NF) if r.want.kinds[n] != "copy"][:1]
    odd = {n: [ODD[(np.arange(p.size) + n) % ODD.size].reshape(p.shape).view(F) for p in r.floats[n]] for n in copies}
    src = [mv.frame_to_device(odd[n]) if n in odd else r.src[n] for n in range(fx.NF)]
    out = r.run(r.make(), copies + usable, src=src)
    torch.cuda.synchronize()
    for k, n in enumerate(copies):
        _same(mv, out[k], odd[n], "the copied frame %d" % n)
    _same(mv, out[len(copies)], r.want.frames[usable[0]], "the compensated frame %d" % usable[0])


# ------------------------------------------------------------------------------------------------ layouts

LAYOUTS = ["tight", "plus1", "offset", "uv_differ"]
FOUR = THREE + [(fx.FLOW_CRAFTED, "35x30-444-limits-shift")]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cases,name", FOUR, ids=["fetch", "shift", "blur", "shift-odd-width"])
def test_planes_carved_out_of_arenas_of_quiet_nans_and_of_two_fills(oracle, mv, cases, name, layout):
    """clip frames and destinations at a tight pitch, a pitch of an odd number of samples, inside a wider frame one sample off a 256-byte
    boundary, with U and V of different pitch -- carved out of arenas of quiet NaNs, 0xA5 and 0x5A: the results are the restatement's, nothing
    but samples is written, and no clip frame changes"""
    import torch
    r = _rig(mv, oracle, _case(cases, name))
    ws, hs_ = [p.shape[1] for p in r.floats[0]], [p.shape[0] for p in r.floats[0]]
    pitch = [lo.clip_layout(layout, w, 4, p)[0] for p, w in enumerate(ws)]
    g = r.make(clip_pitch=pitch, dst_pitch=pitch)
    copy = [n for n in range(fx.NF) if r.want.kinds[n] == "copy"][0]
    ns = [[n for n in range(fx.NF) if r.want.kinds[n] != "copy"][0], copy]
    for fill in (lo.NAN_FILL,) + tuple(lo.FILLS):
        name_ = "NaN fill" if not isinstance(fill, int) else "fill 0x%02x" % fill
        clips = [lo.clip_planes(layout, ws, hs_, 4, fill) for _ in range(fx.NF)]
        for n in range(fx.NF):
            for (_, view), plane in zip(clips[n], r.floats[n]):
                lo.put(view, plane)
        snap = [[a.clone() for a, _ in fr] for fr in clips]
        outs = [lo.clip_planes(layout, ws, hs_, 4, fill) for _ in ns]
        r.run(g, ns, src=[[v for _, v in fr] for fr in clips], out=[[v for _, v in fr] for fr in outs])
        torch.cuda.synchronize()
        for k, n in enumerate(ns):
            _same(mv, [v for _, v in outs[k]], r.want.frames[n], "%s, %s: frame %d" % (layout, name_, n))
            for p, (arena, view) in enumerate(outs[k]):
                damage = lo.intact(arena, view, ws[p] * 4, fill)
                assert not damage, "%s, %s: frame %d plane %d: %s" % (layout, name_, n, p, lo.describe(damage))
        assert all(torch.equal(a, s) for fr, sn in zip(clips, snap) for (a, _), s in zip(fr, sn)), "%s, %s: a clip frame was written" % (layout, name_)


# ------------------------------------------------------------------------------------------------ one handle over unlike calls, poisoned scratch

@pytest.mark.parametrize("poison", [0xA5, 0x5A], ids=lambda v: "poison%02X" % v)
@pytest.mark.parametrize("cases,name", [(fx.FLOW_CRAFTED, "70x54-invalid"), (fx.FLOW_CRAFTED, "70x54-invalid-shift"), (fx.FLOW_SEARCHED, "420-16bit-pel2-8/4-fw-shift"),
                                        (fx.BLUR_CRAFTED, "70x54-invalid")], ids=["fetch", "shift", "shift-searched", "blur"])
def test_one_handle_over_calls_of_1_5_and_2_jobs(oracle, mv, dbg, cases, name, poison):  # noqa: F811
    """the job table, the flags, the cells and -- in shift mode -- the winners are handle scratch that grows with the largest call: a call of
    one usable job, of all five (usable and copying), then of a copying and a usable one, every fresh allocation poisoned, bit for bit after
    every call; then the same frames again into the outputs of the second call"""
    import torch
    dbg("scratch_poison", poison)
    r = _rig(mv, oracle, _case(cases, name))
    g = r.make()
    usable = [n for n in range(fx.NF) if r.want.kinds[n] != "copy"]
    copies = [n for n in range(fx.NF) if r.want.kinds[n] == "copy"]
    kept = None
    for ns, reuse in (([usable[-1]], False), (list(range(fx.NF)), False), ([copies[0], usable[0]], False), ([usable[0], copies[-1]], True)):
        out = r.run(g, ns, out=kept[:len(ns)] if reuse else None)
        torch.cuda.synchronize()
        for k, n in enumerate(ns):
            _same(mv, out[k], r.want.frames[n], "call of %d jobs, frame %d (%s)" % (len(ns), n, r.want.kinds[n]))
        if len(ns) == fx.NF:
            kept = out


# ------------------------------------------------------------------------------------------------ the package, end to end; refusals

def test_torch_float32_planes_end_to_end(oracle, mv):
    """clip frames as plain torch.float32 planes (rows of width samples, no padding): the filters allocate float32 planes by the float pitch"""
    import torch
    for cases, name in THREE:
        r = _rig(mv, oracle, _case(cases, name))
        src = [[torch.from_numpy(np.ascontiguousarray(p)).to("cuda") for p in fr] for fr in r.floats]
        tight = [p.shape[1] * 4 for p in r.floats[0]]
        assert src[0][0].dtype == torch.float32 and src[0][0].stride(0) * 4 == tight[0]
        g = r.make(clip_pitch=tight)
        assert g.is_float and g.dst_pitch == tight
        out = r.run(g, range(fx.NF), src=src)
        torch.cuda.synchronize()
        for n in range(fx.NF):
            assert all(o.dtype == torch.float32 and o.shape == s.shape for o, s in zip(out[n], src[n]))
            for p, o in enumerate(out[n]):
                assert np.array_equal(ff.bits(o.cpu().numpy()), ff.bits(r.want.frames[n][p])), (name, n, p)


def test_refusals_that_need_no_device(oracle, mv):
    r = _rig(mv, oracle, _case(fx.FLOW_SEARCHED, "420-8bit-pel2-8/4-bw"))
    ad = r.vectors[0][0]
    isup = mv.Super(r.c.w, r.c.h, r.c.bits, **fx.super_kwargs(r.c))
    with pytest.raises(mv.MvtoolsError, match="Flow: float super clips are not supported."):
        mv.Flow(r.fsup, ad, fx.NF, r.pitch)
    with pytest.raises(mv.MvtoolsError, match="Flow: the float entry needs a float super clip."):
        mv.Flow(isup, ad, fx.NF, r.pitch, sample_float=True)
    with pytest.raises(mv.MvtoolsError, match="Flow: fields is not supported on float clips."):
        mv.Flow(r.fsup, ad, fx.NF, r.pitch, sample_float=True, fields=1)
    b = _rig(mv, oracle, _case(fx.BLUR_CRAFTED, "70x54-limits-blur50"))
    with pytest.raises(mv.MvtoolsError, match="FlowBlur: float super clips are not supported."):
        mv.FlowBlur(b.fsup, b.vectors[0][0], b.vectors[1][0], fx.NF, b.pitch)
    with pytest.raises(mv.MvtoolsError, match="FlowBlur: the float entry needs a float super clip."):
        mv.FlowBlur(mv.Super(70, 54, 8), b.vectors[0][0], b.vectors[1][0], fx.NF, b.pitch, sample_float=True)
    with pytest.raises(mv.MvtoolsError, match="FlowInter: float super clips are not supported."):
        mv.FlowInter(b.fsup, b.vectors[0][0], b.vectors[1][0], fx.NF, b.pitch)
