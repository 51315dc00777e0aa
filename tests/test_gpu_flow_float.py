"""GPU: FlowInter and FlowFPS on float clips (mvx_flowinter_create_float, mvx_flowfps_create_float) against the numpy restatement
(tests/flow_float_ref.py, anchored to the integer restatement by tests/test_flow_float_ref.py), bit for bit: planes are compared as uint32, so
NaN payloads and signed zeros count.

The rig is that of the other float filters: the float clip is float_clip of the integer clip, the vectors are searched on the integer copy and
never on the float samples, crafted cases rewrite them on the host, and the float super frames are built on the GPU and asserted to be the Super
restatement's (tests/super_float_ref.py) before the restatement runs on them.  The search is mv.Analyse's on the GPU, in every case, and is
asserted to give the oracle's blobs -- the tiny unpadded clips included, whose search once faulted (tests/test_gpu_small_geometry.py).  Every output frame
of a case is a job of ONE call, so copied and blended frames (FlowFPS at time256 0, clip ends, scene changes, invalid blobs) stand beside
interpolated ones in every batch; tests/test_flow_float_cases.py holds the cases to their conditions on the CPU, and the same conditions are
asserted here."""
import numpy as np
import pytest

import flow_float_cases as fx
import flow_float_ref as fl
import layouts as lo
import super_float_ref as sf
from test_gpu_parity import dbg  # noqa: F401  (the fixture that puts a debug option back)

pytestmark = pytest.mark.gpu

F = np.float32
_rigs = {}


class Rig:
    """one case on the device: the oracle's blobs of the integer clip (edited on the host by the case's recipes), the float clip and its
    float super frames, and the restatement's frames for them"""

    def __init__(self, mv, oracle, c):
        import torch
        self.mv, self.c = mv, c
        self.q, self.floats = fx.clips(c)
        kw = fx.super_kwargs(c)
        # the search runs on the GPU, on the integer copy (mv.Super + mv.Analyse), and must give the oracle's blobs
        isup = mv.Super(c.w, c.h, c.bits, **kw)
        isf = isup.build([mv.frame_to_device(f) for f in self.q])
        searched = []
        for (isb, delta), (oad, oblobs) in zip(fx.fields(c), fx.search_oracle(oracle, c, self.q)):
            an = mv.Analyse(isup, num_frames=fx.NF, isb=isb, delta=delta, **fx.mc.analyse_kwargs(c))
            refs = [fx.mc.reference(isb, delta, n) for n in range(fx.NF)]
            blobs = [b.cpu().numpy() for b in an.run([(isf[n], isf[r] if r is not None else None) for n, r in enumerate(refs)])]
            assert all(np.array_equal(b, o) for b, o in zip(blobs, oblobs)), "mv.Analyse differs from the oracle (isb %d, delta %d)" % (isb, delta)
            searched.append((an.ad, blobs))
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
        self.fallbacks = [n for n, k in enumerate(self.want.kinds) if k in fx.FALLBACKS]
        self.usable = [n for n, k in enumerate(self.want.kinds) if k not in fx.FALLBACKS]

    def make(self, clip_pitch=None, dst_pitch=None):
        mv, c = self.mv, self.c
        cls = mv.FlowInter if c.kind == "inter" else mv.FlowFPS
        g = cls(self.fsup, self.vectors[0][0], self.vectors[1][0], fx.NF, clip_pitch or self.pitch, dst_pitch=dst_pitch, sample_float=True, **fx.package_kwargs(c))
        assert g.num_frames == self.want.num_frames and all(g.map(n) == self.want.ref.map(n) for n in range(g.num_frames))
        return g

    def run(self, g, ns, src=None, out=None):
        """output frames ns as the jobs of one call of handle g -> the output frames (device planes)"""
        return g.run(list(ns), src or self.src, self.fsf, self.blobs[0], self.blobs[1], out=out)


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
        a, b = fl.bits(_np(mv, got[p], want[p].shape[1])), fl.bits(want[p])
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
    out = r.run(g, range(g.num_frames))
    torch.cuda.synchronize()
    last = fx.NF - 1
    for n in range(g.num_frames):
        kind = r.want.kinds[n]
        assert all(o.dtype == torch.float32 for o in out[n])
        _same(mv, out[n], r.want.frames[n], "frame %d (%s, time256 %d)" % (n, kind, r.want.times[n]))
        if kind in ("copy", "left"):
            nl, nr, t = g.map(n)
            _same(mv, out[n], r.floats[min(nr if kind == "copy" and t == 256 else nl, last)], "the copied frame %d" % n)


# ------------------------------------------------------------------------------------------------ copies move bits

ODD = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x7F7FFFFF], np.uint32)
COPIERS = [(fx.FPS_SEARCHED, "70x54-16bit-pel2-4/2-60-mask2"), (fx.FPS_CRAFTED, "70x54-scene-60-mask1-blend0"), (fx.INTER_CRAFTED, "70x54-scene-blend0")]


@pytest.mark.parametrize("cases,name", COPIERS, ids=["fps-copy", "fps-left", "inter-left"])
def test_a_copied_frame_keeps_quiet_nans_with_their_payloads(oracle, mv, cases, name):
    """the clip frames that the copying jobs copy (FlowFPS at time256 0; the left frame of a blend 0 fallback) are filled with quiet NaNs of
    several payloads, negative zero, infinities, a denormal: the output is those bits, and the interpolated frame beside them -- which reads
    super frames and never the clip -- is untouched by it"""
    import torch
    r = _rig(mv, oracle, _case(cases, name))
    g = r.make()
    copies = [n for n in range(g.num_frames) if r.want.kinds[n] in ("copy", "left")]
    sources = {n: min(g.map(n)[0], fx.NF - 1) for n in copies}
    usable = r.usable[:1]
    odd = {k: [ODD[(np.arange(p.size) + k) % ODD.size].reshape(p.shape).view(F) for p in r.floats[k]] for k in set(sources.values())}
    src = [mv.frame_to_device(odd[k]) if k in odd else r.src[k] for k in range(fx.NF)]
    out = r.run(g, copies + usable, src=src)
    torch.cuda.synchronize()
    for k, n in enumerate(copies):
        _same(mv, out[k], odd[sources[n]], "the copied frame %d" % n)
    _same(mv, out[len(copies)], r.want.frames[usable[0]], "the interpolated frame %d" % usable[0])


# ------------------------------------------------------------------------------------------------ layouts

LAYOUTS = ["tight", "plus1", "offset", "uv_differ"]
FOUR = [(fx.FPS_SEARCHED, "70x54-16bit-pel2-4/2-60-mask2"), (fx.INTER_CRAFTED, "70x54-invalid"), (fx.FPS_CRAFTED, "35x30-444-4/2-occlusion-48-mask0"),
        (fx.INTER_SEARCHED, "420-8bit-pel2-8/4-time50")]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cases,name", FOUR, ids=["fps-extra", "inter-regular", "fps-simple-odd-width", "inter-segments-of-4"])
def test_planes_carved_out_of_arenas_of_quiet_nans_and_of_two_fills(oracle, mv, cases, name, layout):
    """clip frames and destinations at a tight pitch, a pitch of an odd number of samples, inside a wider frame one sample off a 256-byte
    boundary, with U and V of different pitch -- carved out of arenas of quiet NaNs, 0xA5 and 0x5A: an interpolated, a blended or copied job
    give the restatement's frames, nothing but samples is written, and no clip frame changes"""
    import torch
    r = _rig(mv, oracle, _case(cases, name))
    ws, hs_ = [p.shape[1] for p in r.floats[0]], [p.shape[0] for p in r.floats[0]]
    pitch = [lo.clip_layout(layout, w, 4, p)[0] for p, w in enumerate(ws)]
    g = r.make(clip_pitch=pitch, dst_pitch=pitch)
    blends = [n for n in r.fallbacks if r.want.kinds[n] == "blend"]
    ns = [r.usable[0], (blends or r.fallbacks)[0], r.usable[-1]]
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
            _same(mv, [v for _, v in outs[k]], r.want.frames[n], "%s, %s: frame %d (%s)" % (layout, name_, n, r.want.kinds[n]))
            for p, (arena, view) in enumerate(outs[k]):
                damage = lo.intact(arena, view, ws[p] * 4, fill)
                assert not damage, "%s, %s: frame %d plane %d: %s" % (layout, name_, n, p, lo.describe(damage))
        assert all(torch.equal(a, s) for fr, sn in zip(clips, snap) for (a, _), s in zip(fr, sn)), "%s, %s: a clip frame was written" % (layout, name_)


# ------------------------------------------------------------------------------------------------ one handle over unlike calls, poisoned scratch

@pytest.mark.parametrize("poison", [0xA5, 0x5A], ids=lambda v: "poison%02X" % v)
@pytest.mark.parametrize("cases,name", [(fx.INTER_CRAFTED, "70x54-invalid"), (fx.FPS_CRAFTED, "70x54-invalid-60-mask2"), (fx.FPS_CRAFTED, "96x64-occlusion-48-mask2")],
                         ids=["inter", "fps", "fps-occlusion"])
def test_one_handle_over_calls_of_1_all_and_2_jobs(oracle, mv, dbg, cases, name, poison):  # noqa: F811
    """the job table, the flags, the small masks, the cells and the mask bytes are handle scratch that grows with the largest call: a call of
    one interpolated job, of all (interpolated, blended and copied), then of a fallback and an interpolated one, every fresh allocation
    poisoned, bit for bit after every call; then two frames again into the outputs of the second call"""
    import torch
    dbg("scratch_poison", poison)
    r = _rig(mv, oracle, _case(cases, name))
    g = r.make()
    usable, fallbacks, every = r.usable, r.fallbacks, list(range(r.want.num_frames))
    kept = None
    for ns, reuse in (([usable[-1]], False), (every, False), ([fallbacks[0], usable[0]], False), ([usable[0], fallbacks[-1]], True)):
        out = r.run(g, ns, out=kept[:len(ns)] if reuse else None)
        torch.cuda.synchronize()
        for k, n in enumerate(ns):
            _same(mv, out[k], r.want.frames[n], "call of %d jobs, frame %d (%s)" % (len(ns), n, r.want.kinds[n]))
        if len(ns) == len(every):
            kept = out


# ------------------------------------------------------------------------------------------------ the package, end to end

def test_torch_float32_planes_end_to_end(oracle, mv):
    """clip frames as plain torch.float32 planes (rows of width samples, no padding): the filters allocate float32 planes by the float pitch"""
    import torch
    for cases, name in FOUR[:3]:
        r = _rig(mv, oracle, _case(cases, name))
        src = [[torch.from_numpy(np.ascontiguousarray(p)).to("cuda") for p in fr] for fr in r.floats]
        tight = [p.shape[1] * 4 for p in r.floats[0]]
        assert src[0][0].dtype == torch.float32 and src[0][0].stride(0) * 4 == tight[0]
        g = r.make(clip_pitch=tight)
        assert g.is_float and g.dst_pitch == tight
        out = r.run(g, range(g.num_frames), src=src)
        torch.cuda.synchronize()
        for n in range(g.num_frames):
            assert all(o.dtype == torch.float32 and o.shape == s.shape for o, s in zip(out[n], src[0]))
            for p, o in enumerate(out[n]):
                assert np.array_equal(fl.bits(o.cpu().numpy()), fl.bits(r.want.frames[n][p])), (name, n, p)
