"""GPU: the block filters, Super, Finest, Analyse and Recalculate in the plane layouts that include/mvtools_amd.h ("Plane layouts") allows,
not only in the one layout every other GPU test uses (rows padded to 256 bytes, planes on 256-byte boundaries of a zero-filled arena).

Every plane, super frame and blob is carved out of an arena filled with 0xA5 or 0x5A (tests/layouts.py): clip planes at a tight pitch, a
pitch of one sample more than a row (odd at 8 bits, 2 mod 4 at 16), at bases one and three samples off a 256-byte boundary, with U and V of
different pitch; super frames at pitches of 16 mod 32 and 16 mod 256 on 16-byte boundaries.  In a run the inputs, super frames and blobs hold
one fill and the output planes the other, so that a row tail copied from an input into an output shows too.  Every case asserts, under BOTH fills,
  - the samples equal the CPU oracle's (or, for DegrainN, the numpy restatement's), byte for byte;
  - no byte of a destination arena that is not a sample changed (row tails, guard rows, the bytes behind a blob, and for Super every byte of
    the super frame outside the defined rectangles);
  - no byte of an input arena changed at all.
Read-independence needs no assertion of its own: a kernel that read a byte nobody wrote -- a row tail, a super-frame byte outside the defined
rectangles, a pad byte behind a blob -- would see 0xA5 in one run and 0x5A in the other and could equal the oracle in at most one of them.

The yardstick is computed once per case on the CPU and shared by the layouts of the case (_oracle).

Super: which kernels serve a layout is decided per level in mvx_super_frames (csrc/mvx_super.hip, `rows` / `rowsOk`): the rows-in-registers
kernels need src_pitch % 4 == 0, dword-aligned source planes and 16-byte aligned destination planes, everything else takes the tile kernels.
So at 206 x 118, 8 bits, `tight` (pitch 206, 2 mod 4), `plus1` (207) and the `offset` layouts (bases 1 and 3) take the tile path and `padded`
and `uv_differ` the rows path; no debug statistic exposes the choice, so it is stated here from the code and both must equal the oracle.

The float Super and the float DegrainN run in the float layouts (pitches and bases multiples of 4, super planes of 16) under the two fills and
under a third whose every non-sample dword is the float32 quiet NaN, with np.array_equal on float32; their refusals of an off-by-2 pitch or base
are checked here to write nothing (the messages also in tests/test_float_host.py).

Layouts dropped to keep the file at a few hundred cases -- never `tight` or `offset`, which every filter gets as a source (where it reads clip
planes) AND as a destination:
  - Degrain radius 1 at 8/4 and 16/8 (both sizes) and radius 3 at 8 bits run all eleven rows of BLOCK_LAYOUTS; radius 3 at 16 bits, the two
    side-by-side cases, the plane=0 case and BlockFPS run SIX_LAYOUTS: dropped are the rows plus1 -> plus1, offset -> plus1, offset3 -> offset3,
    uv_differ -> tight and padded -> offset, so `uv_differ` is never a source and `plus1` and `offset3` are never destinations there;
  - the Flow filters run FLOW_LAYOUTS: dropped in addition tight -> tight (a tight source and a tight destination stay, in different rows), kept
    uv_differ -> tight (`plus1` and `offset3` are never destinations);
  - the 64/32 Degrain case and the radius-7 DegrainN cases run SHORT_LAYOUTS: no `plus1`, `offset3` or `uv_differ` on either side;
  - Compensate and CompensateN read no clip plane: their tables name destinations only (Compensate all six, CompensateN padded, tight, plus1, offset);
  - Analyse and Recalculate take super layouts only: the control, sup16 and sup256.
Over all 83 Degrain cases source and destination differ in 53."""
import numpy as np
import pytest

import degrain_n_cases as dc
import layouts as lo
import pipeline as pl
import test_gpu_parity as tp
from test_gpu_parity import dbg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

_oracle = {}


def _cached(key, make):
    if key not in _oracle:
        _oracle[key] = make()
    return _oracle[key]


def _kw(d):
    return tuple(sorted(d.items()))


class Rig:
    """One clip on the device in a layout: its frames, its super frames built by the GPU into filled arenas, searched blobs in filled arenas.
    Everything registered as an input is compared with its snapshot by unchanged()."""

    def __init__(self, mv, frames, w, h, bits, skw, fill, src_layout="padded", sup_layout=None, build=True):
        probe = mv.Super(w, h, bits, **skw)
        self.mv, self.fill, self.frames = mv, fill, frames
        self.out_fill = fill ^ 0xFF if isinstance(fill, int) else fill  # output planes hold the OTHER fill (0xA5 ^ 0xFF == 0x5A): a row tail copied from an input to an output shows
        self.bps, self.dtype = probe.bps, probe.dtype
        self.sup = probe
        if sup_layout:
            self.sup = mv.Super(w, h, bits, pitch=[lo.super_pitch(sup_layout, probe.info.plane_width[p] * probe.bps) for p in range(probe.nplanes)], **skw)
        self.sup_residue = lo.super_residue(sup_layout) if sup_layout else 0
        self.inputs, self.analyses = [], {}
        self.src = [self.clip_frame(src_layout, f, "src frame %d" % i)[0] for i, f in enumerate(frames)]
        self.src_pitch = [p.stride(0) for p in self.src[0]]
        self.sf, self.sf_arenas = [], []
        if build:
            for _ in frames:
                fr, ar = self.super_frame()
                self.sf.append(fr)
                self.sf_arenas.append(ar)
            self.sup.build(self.src, out=self.sf)
            for i, ar in enumerate(self.sf_arenas):
                self.inputs += [("super frame %d plane %d" % (i, p), a) for p, a in enumerate(ar)]

    # ---- carving
    def clip_frame(self, layout, planes=None, what=None, shapes=None, bps=None):
        """a frame in a clip-side layout holding `planes` (an input, registered) or of `shapes` (rows, width), an output -> (views, guards)"""
        bps = bps or self.bps
        views, guards = [], []
        fill = self.fill if planes is not None else self.out_fill
        for p, shape in enumerate([a.shape for a in planes] if planes is not None else shapes):
            pitch, residue = lo.clip_layout(layout, shape[1], bps, p)
            arena, view = lo.carve(shape[0], shape[1] * bps, pitch, residue, fill)
            if planes is not None:
                lo.put(view, planes[p])
                self.inputs.append(("%s plane %d" % (what, p), arena))
            views.append(view)
            guards.append((arena, view, shape[1] * bps, fill))
        return views, guards

    def super_frame(self):
        """a super frame of self.sup's layout (with room for its shadow planes) inside filled arenas -> (planes, arenas)"""
        s = self.sup
        planes, arenas = [], []
        for p in range(s.nplanes):
            total = s.shadow_stride[p] * s.slots[p]
            arena, view = lo.carve(1, total, total, self.sup_residue, self.fill)
            h = s.info.plane_height[p]
            planes.append(view[0][:h * s.pitch[p]].view(h, s.pitch[p]))
            arenas.append(arena)
        return planes, arenas

    def blobs(self, n, size):
        """n blobs of `size` bytes at 16-byte aligned addresses of filled arenas -> (blobs, guards)"""
        out, guards = [], []
        for _ in range(n):
            arena, view = lo.carve(1, size, lo.ceil_to(size, 16) + 16, 16, self.fill, guard_rows=1)
            out.append(view[0][:size])
            guards.append((arena, view, size, self.fill))
        return out, guards

    # ---- running
    def analyse(self, **akw):
        key = _kw(akw)
        if key not in self.analyses:
            self.analyses[key] = self.mv.Analyse(self.sup, **akw)
        return self.analyses[key]

    def search(self, an, jobs, want=None, field_shift=0):
        """jobs of (source frame number, reference frame number or None) searched into carved blobs; with `want` (the oracle's blobs) they
        are checked here, and always the bytes behind them.  The blobs become inputs."""
        blobs, guards = self.blobs(len(jobs), an.blob_size)
        an.run([(self.sf[s], self.sf[r] if r is not None else None) for s, r in jobs], blobs=blobs, field_shift=field_shift)
        self.sync()
        for i, (arena, view, size, _) in enumerate(guards):
            if want is not None:
                assert np.array_equal(blobs[i].cpu().numpy(), want[i]), "fill 0x%02x: blob %d differs from the oracle's" % (self.fill, i)
            _intact("blob %d" % i, self.fill, [guards[i]], guard_rows=1)
            self.inputs.append(("blob %d" % i, arena))
        return blobs

    def sync(self):
        import torch
        torch.cuda.synchronize()

    def freeze(self):
        self.snap = [a.clone() for _, a in self.inputs]

    def unchanged(self):
        import torch
        for (what, a), s in zip(self.inputs, self.snap):
            if not torch.equal(a, s):
                i = int(torch.nonzero(a != s)[0])
                pytest.fail("fill 0x%02x: input %s was written: arena byte %d was 0x%02x, is 0x%02x" % (self.fill, what, i, int(s[i]), int(a[i])))


def _intact(what, fill, guards, guard_rows=8):
    """`fill` names the run in the message; every guard carries the fill of its own arena"""
    for p, (arena, view, row_bytes, own) in enumerate(guards):
        damage = lo.intact(arena, view, row_bytes, own, guard_rows=guard_rows)
        assert not damage, "fill 0x%02x: %s plane %d: %s" % (fill, what, p, lo.describe(damage))


def _same(what, fill, views, want):
    for p in range(len(want)):
        got = lo.get(views[p], want[p].shape[1], want[p].dtype)
        assert pl.first_diff(got, want[p]) == "", "fill 0x%02x: %s plane %d: %s" % (fill, what, p, pl.first_diff(got, want[p]))


# src layout, dst layout, super layout: `padded, padded, default` is the control.  src and dst differ in 7 of the 11 rows; every one of the six
# layouts is a source in some row and a destination in some row.
BLOCK_LAYOUTS = [
    ("padded", "padded", None),
    ("tight", "tight", None),
    ("tight", "offset", "sup16"),
    ("plus1", "tight", "sup256"),
    ("plus1", "plus1", None),
    ("offset", "tight", None),
    ("offset", "plus1", "sup16"),
    ("offset3", "uv_differ", "sup256"),
    ("offset3", "offset3", None),
    ("uv_differ", "tight", None),
    ("padded", "offset", None),
]
# the shorter tables keep `tight` and `offset` on BOTH sides: a tight and an offset source, a tight and an offset destination
SIX_LAYOUTS = [BLOCK_LAYOUTS[i] for i in (0, 1, 2, 3, 5, 7)]     # src != dst in 4 of 6: + plus1 -> tight on sup256, offset -> tight, offset3 -> uv_differ
SHORT_LAYOUTS = [BLOCK_LAYOUTS[i] for i in (0, 1, 2, 5)]         # src != dst in 2 of 4: the control, tight, tight -> offset on sup16, offset -> tight
FLOW_LAYOUTS = [BLOCK_LAYOUTS[i] for i in (0, 2, 3, 5, 7, 9)]    # src != dst in 5 of 6: as SIX_LAYOUTS with uv_differ -> tight for tight -> tight
_lid = lambda l: "%s-%s-%s" % (l[0], l[1], l[2] or "sup")


# ================================================================================================ Super

SUPER_CASES = [
    # w, h, bits, super kwargs, shadow
    (206, 118, 8, {}, None),
    (206, 118, 8, dict(pel=1), None),
    (206, 118, 8, dict(pel=4), None),
    (206, 118, 8, dict(sharp=0), None),
    (206, 118, 8, dict(sharp=1), None),
    (206, 118, 10, {}, None),
    (206, 118, 16, {}, True),
    (206, 118, 16, {}, False),
    (208, 120, 8, {}, None),
    (208, 120, 16, dict(pel=4), True),
]
# src layout (clip side), dst layout (super side)
SUPER_LAYOUTS = [("padded", None), ("tight", None), ("tight", "sup16"), ("plus1", "sup256"), ("offset", "sup16"), ("offset3", "sup256"),
                 ("uv_differ", None)]


def _super_damage(osup, rig, i):
    """the bytes of super frame i that changed although they lie outside the defined rectangles (and outside the shadow planes)"""
    s = rig.sup
    for p in range(s.nplanes):
        arena, plane = rig.sf_arenas[i][p], rig.sf[i][p]
        start = plane.data_ptr() - arena.data_ptr()
        h, pitch = plane.shape
        bad = arena != lo._pattern(rig.fill, arena.data_ptr(), arena.numel(), arena.device)
        area = bad[start:start + h * pitch].view(h, pitch)
        for (q, _lv, _k, y0, x0, hh, ww) in osup.defined_regions():
            if q == p:
                area[y0:y0 + hh, x0 * rig.bps:(x0 + ww) * rig.bps] = False
        if s.slots[p] > 1:  # the shadow planes behind the plane are the library's to write
            bad[start + h * pitch:start + s.shadow_stride[p] * s.slots[p]] = False
        if bool(bad.any()):
            import torch
            j = int(torch.nonzero(bad)[0]) - start
            return "plane %d: byte at row %d, column %d (pitch %d) is outside every defined rectangle and was written" % (p, j // pitch, j % pitch, pitch)
    return ""


@pytest.mark.parametrize("layout", SUPER_LAYOUTS, ids=lambda l: "%s-%s" % (l[0], l[1] or "sup"))
@pytest.mark.parametrize("w,h,bits,skw,shadow", SUPER_CASES)
def test_super(oracle, mv, w, h, bits, skw, shadow, layout):
    def make():
        frames = pl.moving_clip(w, h, bits, 2, seed=5, noise=3)
        osup = oracle.Super(w, h, bits, **skw)
        return frames, osup, [osup.frame(f) for f in frames]
    frames, osup, osf = _cached(("super", w, h, bits, _kw(skw)), make)
    kw = dict(skw) if shadow is None else dict(skw, shadow=shadow)
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, kw, fill, layout[0], layout[1], build=False)
        rig.freeze()
        for _ in frames:
            fr, ar = rig.super_frame()
            rig.sf.append(fr)
            rig.sf_arenas.append(ar)
        rig.sup.build(rig.src, out=rig.sf)
        rig.sync()
        for i in range(len(frames)):
            got = [lo.get(rig.sf[i][p], rig.sup.info.plane_width[p], rig.dtype) for p in range(3)]
            assert pl.defined_equal(osup, osf[i], got) == [], "fill 0x%02x frame %d" % (fill, i)
            assert _super_damage(osup, rig, i) == "", "fill 0x%02x frame %d" % (fill, i)
        rig.unchanged()


# ================================================================================================ Finest

@pytest.mark.parametrize("layout", ["padded", "tight", "plus1", "offset", "offset3", "uv_differ"])
@pytest.mark.parametrize("w,h,bits,pel", [(206, 118, 8, 2), (206, 118, 16, 2), (208, 120, 8, 4), (206, 118, 16, 4)])
def test_finest(oracle, mv, w, h, bits, pel, layout):
    skw = dict(pel=pel)

    def make():
        frames = pl.moving_clip(w, h, bits, 1, seed=6, noise=3)
        osup = oracle.Super(w, h, bits, **skw)
        return frames, osup.finest(osup.frame(frames[0]))
    frames, want = _cached(("finest", w, h, bits, pel), make)
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, skw, fill, "padded", "sup16" if layout in ("tight", "offset") else None)
        dst, guards = rig.clip_frame(layout, shapes=[a.shape for a in want])
        rig.freeze()
        rig.sup.finest(rig.sf, out=[dst])
        rig.sync()
        _same("Finest", fill, dst, want)
        _intact("Finest", fill, guards)
        rig.unchanged()


# ================================================================================================ Analyse, Recalculate

ANALYSE_CASES = [
    # name, w, h, bits, analyse kwargs, debug switches
    ("lean8", 206, 118, 8, dict(blksize=8, overlap=4), dict(spec=0)),
    ("u16-shadow", 206, 118, 16, dict(blksize=16, overlap=8), dict(spec=0)),
    ("generic", 256, 128, 8, dict(blksize=32, overlap=16), {}),
    ("default8", 208, 120, 8, dict(blksize=8, overlap=4), dict(team=0)),
    ("default16", 208, 120, 16, dict(blksize=16, overlap=8), dict(team=0)),
    ("team", 208, 120, 16, dict(blksize=16, overlap=8), dict(spec=5, team=4)),
]
ANALYSE_LAYOUTS = [("padded", None), ("tight", "sup16"), ("offset", "sup256"), ("padded", "sup16")]


@pytest.mark.parametrize("layout", ANALYSE_LAYOUTS, ids=lambda l: "%s-%s" % (l[0], l[1] or "sup"))
@pytest.mark.parametrize("name,w,h,bits,akw,switches", ANALYSE_CASES, ids=[c[0] for c in ANALYSE_CASES])
def test_analyse(oracle, mv, dbg, name, w, h, bits, akw, switches, layout):
    jobs = [(1, 2, 1), (1, 0, 0), (1, None, 1)]  # source, reference, isb

    def make():
        frames = pl.moving_clip(w, h, bits, 3, seed=17, noise=3, motion=(5, -2))
        osup = oracle.Super(w, h, bits)
        osf = [osup.frame(f) for f in frames]
        return frames, [oracle.Analyse(osup, isb=isb, **akw).frame(osf[s], osf[r] if r is not None else None) for s, r, isb in jobs]
    frames, want = _cached(("analyse", w, h, bits, _kw(akw)), make)
    for k, v in switches.items():
        dbg(k, v)
    import ctypes
    info = (ctypes.c_int * 5)()
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, {}, fill, layout[0], layout[1])
        rig.freeze()
        for (s, r, isb), wb in zip(jobs, want):
            rig.search(rig.analyse(isb=isb, **akw), [(s, r)], [wb])
            if name != "generic":  # the kernel the case is meant to cover: 0 serial, 2 speculative, 3 its team form
                mv.lib().mvx_debug_last_launch(info)
                assert info[4] == dict(lean8=0, team=3).get(name, 0 if "spec" in switches else 2), "not the kernel of this case: %s" % list(info)
        rig.unchanged()


@pytest.mark.parametrize("layout", ANALYSE_LAYOUTS, ids=lambda l: "%s-%s" % (l[0], l[1] or "sup"))
@pytest.mark.parametrize("bits,akw,rkw", [(8, dict(blksize=16, overlap=8), dict(blksize=8, overlap=4)), (16, dict(blksize=16, overlap=8), dict(blksize=8, overlap=4)),
                                          (8, dict(blksize=16, overlap=8), dict(blksize=8, overlap=4, divide=2))])
def test_recalculate(oracle, mv, bits, akw, rkw, layout):
    w, h = 206, 118

    def make():
        frames = pl.moving_clip(w, h, bits, 2, seed=51, noise=3)
        osup = oracle.Super(w, h, bits)
        osf = [osup.frame(f) for f in frames]
        oan = oracle.Analyse(osup, isb=1, **akw)
        old = oan.frame(osf[0], osf[1])
        return frames, old, oracle.Recalculate(osup, oan.ad, **rkw).frame(osf[0], osf[1], old)
    frames, old, want = _cached(("recalculate", bits, _kw(akw), _kw(rkw)), make)
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, {}, fill, layout[0], layout[1])
        an = rig.analyse(isb=1, **akw)
        olds = rig.search(an, [(0, 1)], [old])
        rec = mv.Recalculate(rig.sup, an.ad, **rkw)
        blobs, guards = rig.blobs(1, rec.blob_size)
        rig.freeze()
        rec.run([(rig.sf[0], rig.sf[1], olds[0])], blobs=blobs)
        rig.sync()
        assert np.array_equal(blobs[0].cpu().numpy(), want), "fill 0x%02x" % fill
        _intact("recalculated blob", fill, guards, guard_rows=1)
        rig.unchanged()


# ================================================================================================ Degrain

DEGRAIN_CASES = [
    # w, h, bits, radius, analyse kwargs, degrain kwargs, layouts
    (206, 118, 8, 1, dict(blksize=8, overlap=4), {}, BLOCK_LAYOUTS),       # two references: the cell kernel; cells of 4 (chroma 2), live uncovered strips
    (208, 120, 8, 1, dict(blksize=8, overlap=4), {}, BLOCK_LAYOUTS),       # every whole-vector store ends exactly on the width
    (206, 118, 16, 1, dict(blksize=16, overlap=8), {}, BLOCK_LAYOUTS),
    (208, 120, 16, 1, dict(blksize=16, overlap=8), {}, BLOCK_LAYOUTS),
    (270, 72, 8, 3, dict(blksize=8, overlap=4), {}, BLOCK_LAYOUTS),        # six references: the tiled plan, 32 cells x 8 rows, three tile columns, the last partial
    (270, 72, 16, 3, dict(blksize=8, overlap=4), {}, SIX_LAYOUTS),
    (206, 118, 8, 1, dict(blksize=8, overlap=0), {}, SIX_LAYOUTS),         # side by side: cells of 8 (chroma 4)
    (208, 120, 16, 1, dict(blksize=16, overlap=0), {}, SIX_LAYOUTS),
    (256, 128, 8, 1, dict(blksize=64, overlap=32), {}, SHORT_LAYOUTS),     # the per-sample gather
    (206, 118, 8, 1, dict(blksize=8, overlap=4), dict(plane=0), SIX_LAYOUTS),  # luma only: the chroma destination is the source, its tails intact
]


def _degrain_oracle(oracle, w, h, bits, radius, akw, dkw, seed=21):
    """frames, per target (middle frame; frame 0, whose forward references lie outside the clip): reference frame numbers, oracle blobs, oracle output"""
    frames, osup, _, osf, _, _ = tp._pipeline(oracle, _NoGpu, w, h, bits, radius, {}, akw, seed=seed)
    n, targets = len(frames), []
    for target in (radius, 0):
        nrefs, blobs = [], []
        for _, isb, d, nref in dc.neighbours(target, radius, n):
            oan = oracle.Analyse(osup, isb=isb, delta=d, **akw)
            blobs.append(oan.frame(osf[target], osf[nref] if nref is not None else None))
            nrefs.append(nref)
        want = oracle.Degrain(radius, osup, oan.ad, **dkw).frame(frames[target], [osf[r] if r is not None else None for r in nrefs], blobs)
        targets.append((target, nrefs, blobs, want))
    return frames, targets, [[np.ascontiguousarray(fr[p][:, :osup.plane_shape(p)[1]]) for p in range(3)] for fr in osf]


class _NoGpu:
    """stands in for the product binding in tests/test_gpu_parity.py's _pipeline, whose oracle half is all these tests take from it: the
    device half is built per layout and fill by Rig"""
    class Super:
        def __init__(self, *a, **kw):
            pass

        def build(self, frames):
            return None

    @staticmethod
    def frame_to_device(f):
        return None


def _gpu_searches(rig, target, nrefs, oblobs, radius, akw):
    """the GPU's vectors of one Degrain job in carved blobs, checked against the oracle's -> (blobs, analysis data)"""
    blobs = []
    for (_, isb, d, nref), want in zip(dc.neighbours(target, radius, len(rig.frames)), oblobs):
        an = rig.analyse(isb=isb, delta=d, **akw)
        blobs += rig.search(an, [(target, nref)], [want])
    return blobs, an.ad


def _degrain_params():
    return [pytest.param(*c[:6], l, id="%dx%d-%dbit-r%d-%s-%s-%s" % (c[0], c[1], c[2], c[3], ",".join("%s=%s" % kv for kv in _kw(c[4])),
                                                                  ",".join("%s=%s" % kv for kv in _kw(c[5])) or "default", _lid(l))) for c in DEGRAIN_CASES for l in c[6]]


@pytest.mark.parametrize("w,h,bits,radius,akw,dkw,layout", _degrain_params())
def test_degrain(oracle, mv, w, h, bits, radius, akw, dkw, layout):
    frames, targets, _ = _cached(("degrain", w, h, bits, radius, _kw(akw), _kw(dkw)), lambda: _degrain_oracle(oracle, w, h, bits, radius, akw, dkw))
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, {}, fill, layout[0], layout[2])
        for target, nrefs, oblobs, want in targets:
            blobs, ad = _gpu_searches(rig, target, nrefs, oblobs, radius, akw)
            dst, guards = rig.clip_frame(layout[1], shapes=[a.shape for a in want])
            dg = mv.Degrain(radius, rig.sup, ad, rig.src_pitch, [v.stride(0) for v in dst], **dkw)
            rig.freeze()
            dg.run([(rig.src[target], [rig.sf[r] if r is not None else None for r in nrefs], blobs)], out=[dst])
            rig.sync()
            _same("Degrain%d target %d" % (radius, target), fill, dst, want)
            _intact("Degrain%d target %d dst" % (radius, target), fill, guards)
            rig.unchanged()


# ================================================================================================ DegrainN

def _degrain_n_oracle(oracle, mv, w, h, bits, radius, akw, dkw):
    """the restatement's output on the oracle's super frames and vectors (the GPU's are checked to equal them)"""
    frames = dc.clip(w, h, bits, 2 * radius + 1)
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    target, nrefs, blobs = radius, [], []
    for _, isb, d, nref in dc.neighbours(target, radius, len(frames)):
        oan = oracle.Analyse(osup, isb=isb, delta=d, **akw)
        blobs.append(oan.frame(osf[target], osf[nref]))
        nrefs.append(nref)
    ad = mv.Analyse(mv.Super(w, h, bits), isb=0, delta=radius, **akw).ad
    info = mv.DegrainN(radius, mv.Super(w, h, bits), ad, [lo.ceil_to(w * (bits + 7) // 8, 256)] * 3, **dkw).info()
    ref = dc.restatement(oracle, radius, ad, info["thsad_d"], info["thsadc_d"], dkw)
    crop = lambda fr: [np.ascontiguousarray(fr[p][:, :osup.plane_shape(p)[1]]) for p in range(3)]
    return frames, nrefs, blobs, ref.frame(frames[target], [crop(osf[r]) for r in nrefs], blobs)


@pytest.mark.parametrize("layout", SHORT_LAYOUTS, ids=_lid)
@pytest.mark.parametrize("w,h,bits,akw", [(206, 118, 8, dict(blksize=8, overlap=4)), (270, 72, 16, dict(blksize=16, overlap=8))])
def test_degrain_n(oracle, mv, w, h, bits, akw, layout):
    radius = 7
    frames, nrefs, oblobs, want = _cached(("degrain_n", w, h, bits, _kw(akw)), lambda: _degrain_n_oracle(oracle, mv, w, h, bits, radius, akw, {}))
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, {}, fill, layout[0], layout[2])
        blobs, ad = _gpu_searches(rig, radius, nrefs, oblobs, radius, akw)
        dst, guards = rig.clip_frame(layout[1], shapes=[a.shape for a in want])
        dg = mv.DegrainN(radius, rig.sup, ad, rig.src_pitch, [v.stride(0) for v in dst])
        rig.freeze()
        dg.run([(rig.src[radius], [rig.sf[r] for r in nrefs], blobs)], out=[dst])
        rig.sync()
        _same("DegrainN", fill, dst, want)
        _intact("DegrainN dst", fill, guards)
        rig.unchanged()


@pytest.mark.parametrize("layout", [("padded", "tight", None), ("tight", "plus1", None), ("offset", "tight", "sup16"), ("offset3", "plus1", "sup256")], ids=_lid)
def test_degrain_n_out16(oracle, mv, layout):
    """out16 beside its guard test at the padded pitch (tests/test_gpu_degrain_out16.py): tight and plus-one-sample destinations of 16-bit
    samples for an 8-bit clip.  Yardstick: the restatement of out16, tests/degrain_out16_ref.py through the thresholds the filter resolved."""
    import degrain_out16_ref as o16
    w, h, bits, radius, akw = 206, 118, 8, 2, dict(blksize=8, overlap=4)
    frames, targets, osf = _cached(("out16", w, h), lambda: _degrain_oracle(oracle, w, h, bits, radius, akw, {}, seed=23))
    target, nrefs, oblobs, _ = targets[0]

    def restated(dg, ad):
        info = dg.info()
        ref = o16.restatement(oracle, radius, ad, info["thsad_d"], info["thsadc_d"], {})
        return o16.frame(ref, frames[target], [osf[r] if r is not None else None for r in nrefs], oblobs)
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, {}, fill, layout[0], layout[2])
        blobs, ad = _gpu_searches(rig, target, nrefs, oblobs, radius, akw)
        shapes = [a.shape for a in frames[target]]
        dst, guards = rig.clip_frame(layout[1], shapes=shapes, bps=2)
        dg = mv.DegrainN(radius, rig.sup, ad, rig.src_pitch, [v.stride(0) for v in dst], out16=True)
        want = _cached(("out16 want", w, h), lambda: restated(dg, ad))
        rig.freeze()
        dg.run([(rig.src[target], [rig.sf[r] if r is not None else None for r in nrefs], blobs)], out=[dst])
        rig.sync()
        _same("DegrainN out16", fill, dst, want)
        _intact("DegrainN out16 dst", fill, guards)
        rig.unchanged()


# ================================================================================================ Compensate

COMP_CASES = [
    # w, h, bits, analyse kwargs, compensate kwargs
    (206, 118, 8, dict(blksize=8, overlap=4), {}),                 # overlapped: the gather
    (206, 118, 16, dict(blksize=16, overlap=8), {}),
    (208, 120, 8, dict(blksize=8, overlap=0), {}),                 # side by side: cells that are plain copies
    (208, 120, 16, dict(blksize=16, overlap=0), {}),
    (208, 120, 8, dict(blksize=4, overlap=0), {}),                 # the smallest segment: chroma blocks of 2
    (206, 118, 8, dict(blksize=8, overlap=0), {}),                 # chroma cells of 2 and an uncovered strip: a cell that starts inside the covered width must lie inside it
    (206, 118, 8, dict(blksize=8, overlap=0), dict(thscd1=20, thscd2=10)),                 # a scene change, scbehavior 1
    (206, 118, 8, dict(blksize=8, overlap=0), dict(thscd1=20, thscd2=10, scbehavior=0)),
    (206, 118, 16, dict(blksize=8, overlap=4), dict(time=40.0)),
]
# dst layout, super layout (Compensate reads no clip plane)
COMP_LAYOUTS = [("padded", None), ("tight", None), ("tight", "sup16"), ("plus1", None), ("offset", "sup256"), ("offset3", None), ("uv_differ", None)]


def _comp_oracle(oracle, w, h, bits, akw, ckw):
    frames, osup, _, osf, _, _ = tp._pipeline(oracle, _NoGpu, w, h, bits, 1, {}, akw, nframes=2)
    oan = oracle.Analyse(osup, isb=1, **akw)
    jobs = []
    for src, ref in ((0, 1), (1, None)):
        blob = oan.frame(osf[src], osf[ref] if ref is not None else None)
        jobs.append((src, ref, blob, oracle.Compensate(osup, oan.ad, **ckw).frame(osf[src], osf[ref] if ref is not None else None, blob)))
    return frames, jobs


@pytest.mark.parametrize("layout", COMP_LAYOUTS, ids=lambda l: "%s-%s" % (l[0], l[1] or "sup"))
@pytest.mark.parametrize("w,h,bits,akw,ckw", COMP_CASES)
def test_compensate(oracle, mv, w, h, bits, akw, ckw, layout):
    frames, jobs = _cached(("compensate", w, h, bits, _kw(akw), _kw(ckw)), lambda: _comp_oracle(oracle, w, h, bits, akw, ckw))
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, {}, fill, "padded", layout[1])
        an = rig.analyse(isb=1, **akw)
        for src, ref, oblob, want in jobs:
            blob = rig.search(an, [(src, ref)], [oblob])[0]
            dst, guards = rig.clip_frame(layout[0], shapes=[a.shape for a in want])
            comp = mv.Compensate(rig.sup, an.ad, [v.stride(0) for v in dst], **ckw)
            rig.freeze()
            comp.run([(rig.sf[src], rig.sf[ref] if ref is not None else None, blob)], out=[dst])
            rig.sync()
            _same("Compensate %d <- %s" % (src, ref), fill, dst, want)
            _intact("Compensate dst", fill, guards)
            rig.unchanged()


# ================================================================================================ BlockFPS

# w, h, bits, analyse kwargs, mode: modes 0, 2, 3 and 6, overlapped and side by side
BLOCKFPS_CASES = [(206, 118, 8, dict(blksize=8, overlap=4), 0), (208, 120, 16, dict(blksize=16, overlap=0), 0), (206, 118, 8, dict(blksize=8, overlap=0), 2),
                  (206, 118, 16, dict(blksize=8, overlap=4), 3), (208, 120, 8, dict(blksize=8, overlap=0), 3), (206, 118, 8, dict(blksize=16, overlap=8), 6),
                  (206, 118, 16, dict(blksize=16, overlap=0), 6), (208, 120, 8, dict(blksize=8, overlap=4), 2)]
NF = 3


def _blockfps_oracle(oracle, w, h, bits, akw, mode):
    frames, osup, _, osf, _, _ = tp._pipeline(oracle, _NoGpu, w, h, bits, 1, {}, akw, nframes=NF, seed=41)
    oabw, oafw = oracle.Analyse(osup, num_frames=NF, isb=1, **akw), oracle.Analyse(osup, num_frames=NF, isb=0, **akw)
    obbw = [oabw.frame(osf[n], osf[n + 1] if n + 1 < NF else None) for n in range(NF)]
    obfw = [oafw.frame(osf[n], osf[n - 1] if n - 1 >= 0 else None) for n in range(NF)]
    ob = oracle.BlockFPS(osup, oabw.ad, oafw.ad, NF, 24, 1, num=60, den=1, mode=mode, ml=50.0)
    return frames, obbw, obfw, [ob.frame(n, frames, osf, obbw, obfw) for n in range(ob.num_frames)]


@pytest.mark.parametrize("layout", SIX_LAYOUTS, ids=_lid)
@pytest.mark.parametrize("w,h,bits,akw,mode", BLOCKFPS_CASES)
def test_blockfps(oracle, mv, w, h, bits, akw, mode, layout):
    frames, obbw, obfw, want = _cached(("blockfps", w, h, bits, _kw(akw), mode), lambda: _blockfps_oracle(oracle, w, h, bits, akw, mode))
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, {}, fill, layout[0], layout[2])
        abw, afw = rig.analyse(num_frames=NF, isb=1, **akw), rig.analyse(num_frames=NF, isb=0, **akw)
        bbw = rig.search(abw, [(n, n + 1 if n + 1 < NF else None) for n in range(NF)], obbw)
        bfw = rig.search(afw, [(n, n - 1 if n - 1 >= 0 else None) for n in range(NF)], obfw)
        outs = [rig.clip_frame(layout[1], shapes=[a.shape for a in wn]) for wn in want]
        gb = mv.BlockFPS(rig.sup, abw.ad, afw.ad, NF, rig.src_pitch, 24, 1, num=60, den=1, mode=mode, ml=50.0, dst_pitch=[v.stride(0) for v in outs[0][0]])
        assert gb.num_frames == len(want)
        rig.freeze()
        gb.run(list(range(gb.num_frames)), rig.src, rig.sf, bbw, bfw, out=[o[0] for o in outs])
        rig.sync()
        for n, (dst, guards) in enumerate(outs):
            _same("BlockFPS frame %d" % n, fill, dst, want[n])
            _intact("BlockFPS frame %d dst" % n, fill, guards)
        rig.unchanged()


# ================================================================================================ FlowInter, FlowFPS, Flow, FlowBlur
# Yardsticks: the numpy restatements tests/flow_ref.py and tests/flowmc_ref.py on the ORACLE's super frames (through its Finest) and vectors; the
# GPU's super frames and vectors are built in the layout under test and must equal the oracle's before the flow stage runs.

FNF = 4
B84, B168, B80 = dict(blksize=8, overlap=4), dict(blksize=16, overlap=8), dict(blksize=8, overlap=0)


def _flow_clip(oracle, mv, w, h, bits, seed):
    def make():
        frames = pl.moving_clip(w, h, bits, FNF, seed=seed, noise=3)
        osup = oracle.Super(w, h, bits)
        osf = [osup.frame(f) for f in frames]
        crop = [[np.ascontiguousarray(fr[p][:, :osup.plane_shape(p)[1]]) for p in range(3)] for fr in osf]
        finest = {}

        def fin(k):
            if k not in finest:
                finest[k] = osup.finest(crop[k])
            return finest[k]
        info = mv.Super(w, h, bits).info
        return dict(frames=frames, osup=osup, osf=osf, fin=fin, hpad=info.hpad, vpad=info.vpad)
    return _cached(("flow clip", w, h, bits, seed), make)


def _flow_pair(oracle, mv, c, w, h, bits, akw):
    """the two vector clips of a clip: oracle blobs at every frame and the analysis data"""
    def make():
        osup, osf = c["osup"], c["osf"]
        oabw, oafw = oracle.Analyse(osup, num_frames=FNF, isb=1, **akw), oracle.Analyse(osup, num_frames=FNF, isb=0, **akw)
        obbw = [oabw.frame(osf[n], osf[n + 1] if n + 1 < FNF else None) for n in range(FNF)]
        obfw = [oafw.frame(osf[n], osf[n - 1] if n - 1 >= 0 else None) for n in range(FNF)]
        gsup = mv.Super(w, h, bits)
        return obbw, obfw, mv.Analyse(gsup, num_frames=FNF, isb=1, **akw).ad, mv.Analyse(gsup, num_frames=FNF, isb=0, **akw).ad
    return _cached(("flow pair", w, h, bits, _kw(akw), id(c)), make)


def _gpu_pair(rig, akw, obbw, obfw):
    abw, afw = rig.analyse(num_frames=FNF, isb=1, **akw), rig.analyse(num_frames=FNF, isb=0, **akw)
    bbw = rig.search(abw, [(n, n + 1 if n + 1 < FNF else None) for n in range(FNF)], obbw)
    bfw = rig.search(afw, [(n, n - 1 if n - 1 >= 0 else None) for n in range(FNF)], obfw)
    return abw, afw, bbw, bfw


def _check_outputs(rig, what, outs, want):
    rig.sync()
    for n, (dst, guards) in enumerate(outs):
        _same("%s frame %d" % (what, n), rig.fill, dst, want[n])
        _intact("%s frame %d dst" % (what, n), rig.fill, guards)
    rig.unchanged()


@pytest.mark.parametrize("layout", FLOW_LAYOUTS, ids=_lid)
@pytest.mark.parametrize("w,h,bits,akw,fkw", [(206, 118, 8, B84, dict(time=50.0)), (208, 120, 16, B168, dict(time=33.0)),
                                             (206, 118, 8, B84, dict(fps=1, num=60, mask=0)), (208, 120, 16, B84, dict(fps=1, num=60, mask=0)),
                                             (206, 118, 8, B84, dict(fps=1, num=60, mask=2)), (206, 118, 16, B168, dict(fps=1, num=60, mask=2))])
def test_flowinter_flowfps(oracle, mv, w, h, bits, akw, fkw, layout):
    import flow_ref
    c = _flow_clip(oracle, mv, w, h, bits, 91)
    obbw, obfw, adbw, adfw = _flow_pair(oracle, mv, c, w, h, bits, akw)
    fkw = dict(fkw)
    fps = fkw.pop("fps", None)

    def make():
        ref = flow_ref.Flow(adbw, adfw, FNF, 3, c["hpad"], c["vpad"], **(dict(fkw, fps=(24, 1)) if fps else fkw))
        return [ref.frame(n, c["frames"], c["fin"], obbw, obfw) for n in range(ref.num_frames if fps else FNF)]
    want = _cached(("flow", w, h, bits, _kw(akw), _kw(fkw), fps), make)
    for fill in lo.FILLS:
        rig = Rig(mv, c["frames"], w, h, bits, {}, fill, layout[0], layout[2])
        abw, afw, bbw, bfw = _gpu_pair(rig, akw, obbw, obfw)
        outs = [rig.clip_frame(layout[1], shapes=[a.shape for a in wn]) for wn in want]
        dpitch = [v.stride(0) for v in outs[0][0]]
        g = mv.FlowFPS(rig.sup, abw.ad, afw.ad, FNF, rig.src_pitch, 24, 1, dst_pitch=dpitch, **fkw) if fps else \
            mv.FlowInter(rig.sup, abw.ad, afw.ad, FNF, rig.src_pitch, dst_pitch=dpitch, **fkw)
        assert g.num_frames == len(want)
        rig.freeze()
        g.run(list(range(len(want))), rig.src, rig.sf, bbw, bfw, out=[o[0] for o in outs])
        _check_outputs(rig, "FlowFPS" if fps else "FlowInter", outs, want)


@pytest.mark.parametrize("layout", FLOW_LAYOUTS, ids=_lid)
@pytest.mark.parametrize("w,h,bits,akw,isb,fkw", [(206, 118, 8, B84, 1, dict(time=100.0)), (206, 118, 16, B84, 0, dict(time=100.0, mode=1)),
                                                 (208, 120, 16, B168, 1, dict(time=75.0)), (208, 120, 8, B80, 0, dict(time=100.0, mode=1))])
def test_flow(oracle, mv, w, h, bits, akw, isb, fkw, layout):
    import flowmc_ref
    c = _flow_clip(oracle, mv, w, h, bits, 101)
    inside = lambda k: 0 <= k < FNF

    def make():
        osup, osf = c["osup"], c["osf"]
        ad = mv.Analyse(mv.Super(w, h, bits), num_frames=FNF, isb=isb, **akw).ad
        ref = flowmc_ref.Flow(ad, FNF, 3, c["hpad"], c["vpad"], bits, **fkw)
        oan = oracle.Analyse(osup, num_frames=FNF, isb=isb, **akw)
        refs = [ref.ref(n) for n in range(FNF)]
        blobs = [oan.frame(osf[n], osf[refs[n]] if inside(refs[n]) else None) for n in range(FNF)]
        return refs, blobs, [ref.frame(n, c["frames"], c["fin"], blobs[n], 0, {}) for n in range(FNF)]
    refs, oblobs, want = _cached(("flowcomp", w, h, bits, _kw(akw), isb, _kw(fkw)), make)
    for fill in lo.FILLS:
        rig = Rig(mv, c["frames"], w, h, bits, {}, fill, layout[0], layout[2])
        an = rig.analyse(num_frames=FNF, isb=isb, **akw)
        blobs = rig.search(an, [(n, refs[n] if inside(refs[n]) else None) for n in range(FNF)], oblobs)
        outs = [rig.clip_frame(layout[1], shapes=[a.shape for a in wn]) for wn in want]
        g = mv.Flow(rig.sup, an.ad, FNF, rig.src_pitch, dst_pitch=[v.stride(0) for v in outs[0][0]], **fkw)
        assert [g.ref(n) for n in range(FNF)] == refs
        rig.freeze()
        g.run([(rig.src[n], rig.sf[refs[n]] if inside(refs[n]) else None, blobs[n], 0) for n in range(FNF)], out=[o[0] for o in outs])
        _check_outputs(rig, "Flow", outs, want)


@pytest.mark.parametrize("layout", FLOW_LAYOUTS, ids=_lid)
@pytest.mark.parametrize("w,h,bits,akw,fkw", [(206, 118, 8, B84, dict(blur=120.0)), (206, 118, 16, B80, dict(blur=200.0))])
def test_flowblur(oracle, mv, w, h, bits, akw, fkw, layout):
    import flowmc_ref
    c = _flow_clip(oracle, mv, w, h, bits, 103)
    obbw, obfw, adbw, adfw = _flow_pair(oracle, mv, c, w, h, bits, akw)

    def make():
        ref = flowmc_ref.FlowBlur(adbw, adfw, FNF, 3, c["hpad"], c["vpad"], bits, **fkw)
        return [ref.frame(n, c["frames"], c["fin"], obbw, obfw, {}) for n in range(FNF)]
    want = _cached(("flowblur", w, h, bits, _kw(akw), _kw(fkw)), make)
    for fill in lo.FILLS:
        rig = Rig(mv, c["frames"], w, h, bits, {}, fill, layout[0], layout[2])
        abw, afw, bbw, bfw = _gpu_pair(rig, akw, obbw, obfw)
        outs = [rig.clip_frame(layout[1], shapes=[a.shape for a in wn]) for wn in want]
        g = mv.FlowBlur(rig.sup, abw.ad, afw.ad, FNF, rig.src_pitch, dst_pitch=[v.stride(0) for v in outs[0][0]], **fkw)
        rig.freeze()
        g.run(list(range(FNF)), rig.src, rig.sf, bbw, bfw, out=[o[0] for o in outs])
        _check_outputs(rig, "FlowBlur", outs, want)


# ================================================================================================ CompensateN

@pytest.mark.parametrize("layout", [("padded", None), ("tight", None), ("plus1", "sup16"), ("offset", "sup256")], ids=lambda l: "%s-%s" % (l[0], l[1] or "sup"))
@pytest.mark.parametrize("bits,akw", [(8, B84), (16, B168)])
def test_compensate_n(oracle, mv, bits, akw, layout):
    """beside its guard test at the padded pitch (tests/test_gpu_multi.py): tr 1 on the middle frame of three; every compensated output is
    the oracle's Compensate for that pair, the centre is the source frame"""
    w, h, n = 206, 118, 1

    def make():
        frames, osup, _, osf, _, _ = tp._pipeline(oracle, _NoGpu, w, h, bits, 1, {}, akw, nframes=3, seed=61)
        fields, wants = [], []
        for r, nref in enumerate(mv.multi_refs(n, 1, 3)):
            oan = oracle.Analyse(osup, num_frames=3, isb=1 - r % 2, delta=r // 2 + 1, **akw)
            fields.append(oan.frame(osf[n], osf[nref]))
            wants.append(oracle.Compensate(osup, oan.ad).frame(osf[n], osf[nref], fields[-1]))
        return frames, fields, wants
    frames, ofields, wants = _cached(("compensate_n", bits), make)
    for fill in lo.FILLS:
        rig = Rig(mv, frames, w, h, bits, {}, fill, "padded", layout[1])
        an = mv.AnalyseN(rig.sup, 1, num_frames=3, **akw)
        blobs, guards = rig.blobs(1, an.blob_size)
        refs = [rig.sf[m] for m in mv.multi_refs(n, 1, 3)]
        an.run([(rig.sf[n], refs)], blobs=blobs)
        rig.sync()
        for r, f in enumerate(an.fields(blobs[0])):
            assert np.array_equal(f.cpu().numpy(), ofields[r]), "fill 0x%02x: field %d differs from the oracle's" % (fill, r)
        _intact("multi blob", fill, guards, guard_rows=1)
        rig.inputs.append(("multi blob", guards[0][0]))
        outs = [rig.clip_frame(layout[0], shapes=[a.shape for a in frames[n]]) for _ in range(3)]
        cn = mv.CompensateN(1, rig.sup, an.ad(0), [v.stride(0) for v in outs[0][0]])
        rig.freeze()
        cn.run([(rig.sf[n], refs, blobs[0])], out=[[o[0] for o in outs]])
        want = []
        for k in range(3):
            _, field = cn.map(k)
            want.append(frames[n] if field < 0 else wants[field])
        _check_outputs(rig, "CompensateN", outs, want)


# ================================================================================================ float Super, float DegrainN

FLOAT_FILLS = list(lo.FILLS) + [lo.NAN_FILL]
FW, FH = 70, 54   # 4:2:0 chroma 35 x 27: odd widths, the scalar tail of the 8-sample store, partial cells
# src layout, dst layout (DegrainN), super layout
FLOAT_LAYOUTS = [("padded", "padded", None), ("tight", "plus1", "sup16"), ("plus1", "tight", "sup256"), ("offset", "offset3", "sup16"), ("offset3", "uv_differ", None),
                 ("uv_differ", "offset", "sup256")]
_fname = lambda f: "fill 0x%02x" % f if isinstance(f, int) else "NaN fill"


def _float_frames(n, seed=5):
    import degrain_float_cases as fc
    q = _cached(("float q", n, seed), lambda: pl.moving_clip(FW, FH, 16, n, seed=seed, noise=3, motion=(1, 0)))
    return q, _cached(("float clip", n, seed), lambda: fc.float_clip(q, 16, seed=2))


def _float_super_damage(rig, i, defined):
    """the first byte of super frame i outside the restatement's defined samples that no longer holds the fill"""
    import torch
    for p in range(rig.sup.nplanes):
        arena, plane = rig.sf_arenas[i][p], rig.sf[i][p]
        start, (h, pitch) = plane.data_ptr() - arena.data_ptr(), plane.shape
        bad = arena != lo._pattern(rig.fill, arena.data_ptr(), arena.numel(), arena.device)
        mask = torch.from_numpy(np.repeat(defined[p], 4, axis=1)).to(arena.device)
        area = bad[start:start + h * pitch].view(h, pitch)
        area[:, :mask.shape[1]] &= ~mask
        if bool(bad.any()):
            j = int(torch.nonzero(bad)[0]) - start
            return "plane %d: byte at row %d, column %d (pitch %d) is outside every defined rectangle and was written" % (p, j // pitch, j % pitch, pitch)
    return ""


@pytest.mark.parametrize("layout", FLOAT_LAYOUTS, ids=_lid)
@pytest.mark.parametrize("pel,sharp", [(1, 2), (2, 2), (2, 1), (4, 0)])
def test_super_float(mv, pel, sharp, layout):
    import super_float_ref as sf
    _, frames = _float_frames(2)
    wants = _cached(("float super", pel, sharp), lambda: [sf.frame(f, pel=pel, sharp=sharp) for f in frames])
    for fill in FLOAT_FILLS:
        rig = Rig(mv, frames, FW, FH, 32, dict(sample_float=True, pel=pel, sharp=sharp), fill, layout[0], layout[2], build=False)
        rig.freeze()
        for _ in frames:
            fr, ar = rig.super_frame()
            rig.sf.append(fr)
            rig.sf_arenas.append(ar)
        rig.sup.build(rig.src, out=rig.sf)
        rig.sync()
        for i, (want, defined) in enumerate(wants):
            for p in range(3):
                got = lo.get(rig.sf[i][p], want[p].shape[1], np.float32)
                assert np.array_equal(got[defined[p]], want[p][defined[p]]), "%s frame %d plane %d: %s" % (
                    _fname(fill), i, p, pl.first_diff(np.where(defined[p], got, 0), want[p]))
            assert _float_super_damage(rig, i, defined) == "", "%s frame %d" % (_fname(fill), i)
        assert all(bool((a == s_).all()) for (_, a), s_ in zip(rig.inputs, rig.snap)), "%s: a source plane was written" % _fname(fill)


@pytest.mark.parametrize("layout", FLOAT_LAYOUTS, ids=_lid)
@pytest.mark.parametrize("radius,akw", [(1, dict(blksize=8, overlap=4)), (2, dict(blksize=16, overlap=8)), (1, dict(blksize=8, overlap=0))])
def test_degrain_n_float(oracle, mv, radius, akw, layout):
    """the vectors are the oracle's search on the 16-bit copy, uploaded; the yardstick is tests/degrain_float_ref.py on the Super restatement's
    frames (tests/test_gpu_super_float.py and test_super_float above hold the GPU's float super frames to it)"""
    import degrain_float_cases as fc
    import super_float_ref as sf
    import torch
    n, target = 2 * radius + 1, radius
    q, frames = _float_frames(n, seed=7)

    def make():
        _, _, ad, nrefs, blobs = fc.oracle_job(oracle, q, FW, FH, 16, radius, target, akw)
        sup_np = [sf.frame(f)[0] for f in frames]
        pad = [lo.ceil_to(FW * 4, 256), lo.ceil_to(FW * 2, 256), lo.ceil_to(FW * 2, 256)]
        info = mv.DegrainN(radius, mv.Super(FW, FH, 32, sample_float=True), ad, pad).info()
        ref = fc.restatement(oracle, radius, ad, info["thsad_d"], info["thsadc_d"], {})
        return ad, nrefs, blobs, ref.frame(frames[target], [sup_np[m] for m in nrefs], blobs)
    ad, nrefs, oblobs, want = _cached(("float degrain", radius, _kw(akw)), make)
    assert not np.array_equal(want[0], frames[target][0])
    for fill in FLOAT_FILLS:
        rig = Rig(mv, frames, FW, FH, 32, dict(sample_float=True), fill, layout[0], layout[2])
        blobs, bguards = rig.blobs(len(oblobs), len(oblobs[0]))
        for b, o, g in zip(blobs, oblobs, bguards):
            b.copy_(torch.from_numpy(np.ascontiguousarray(o)).to(b.device))
            rig.inputs.append(("blob", g[0]))
        dst, guards = rig.clip_frame(layout[1], shapes=[a.shape for a in want])
        dg = mv.DegrainN(radius, rig.sup, ad, rig.src_pitch, [v.stride(0) for v in dst])
        assert dg.is_float and dg.out_bits == 32
        rig.freeze()
        dg.run([(rig.src[target], [rig.sf[m] for m in nrefs], blobs)], out=[dst])
        rig.sync()
        for p in range(3):
            got = lo.get(dst[p], want[p].shape[1], np.float32)
            assert np.array_equal(got, want[p]), "%s plane %d: %s" % (_fname(fill), p, pl.first_diff(got, want[p]))
            damage = lo.intact(*guards[p][:3], guards[p][3])
            assert not damage, "%s dst plane %d: %s" % (_fname(fill), p, lo.describe(damage))
        assert all(bool((a == s_).all()) for (_, a), s_ in zip(rig.inputs, rig.snap)), "%s: an input was written" % _fname(fill)


def test_float_refusals_write_nothing(mv):
    """an off-by-2 source pitch or base: MVX_E_ARG with the documented message, and not a byte of the destination changes"""
    import torch
    _, frames = _float_frames(2)
    fill = 0xA5
    rig = Rig(mv, frames, FW, FH, 32, dict(sample_float=True), fill, "padded", None)
    untouched = lambda arenas: all(bool((a == lo._pattern(fill, a.data_ptr(), a.numel(), a.device)).all()) for a in arenas)
    rows = [a.shape[1] * 4 for a in frames[0]]

    def odd(pitch_extra, residue):
        out = []
        for p, a in enumerate(frames[0]):
            _, view = lo.carve(a.shape[0], rows[p], lo.ceil_to(rows[p], 256) + pitch_extra, residue, fill)
            out.append(view)
        return out
    fr, ar = rig.super_frame()
    with pytest.raises(mv.MvtoolsError, match="float planes need a dst pitch that is a multiple of 16 bytes and a src pitch that is a multiple of 4"):
        rig.sup.build([odd(2, 0)], out=[fr])
    with pytest.raises(mv.MvtoolsError, match=r"float planes must be aligned \(dst to 16 bytes, src to 4\)"):
        rig.sup.build([odd(0, 2)], out=[fr])
    rig.sync()
    assert untouched(ar)
    ad = mv.Analyse(mv.Super(FW, FH, 16), isb=1, blksize=8, overlap=4).ad
    with pytest.raises(mv.MvtoolsError, match="src pitch of plane 0 must hold a row of 280 bytes and be a multiple of the sample size."):
        mv.DegrainN(1, rig.sup, ad, [rig.src_pitch[0] + 2] + rig.src_pitch[1:])
    dg = mv.DegrainN(1, rig.sup, ad, rig.src_pitch)
    dst, guards = rig.clip_frame("padded", shapes=[a.shape for a in frames[0]])
    blobs, _ = rig.blobs(2, mv.lib().mvx_vectors_size(ctypes_ad(mv, ad)))
    with pytest.raises(mv.MvtoolsError, match="mvx_degrain_n_frames: src plane 0 must be aligned to 4 bytes"):
        dg.run([(odd(0, 2), [rig.sf[1], rig.sf[1]], blobs)], out=[dst])
    with pytest.raises(mv.MvtoolsError, match="mvx_degrain_n_frames: dst plane 1 must be aligned to 4 bytes"):
        dg.run([(rig.src[0], [rig.sf[1], rig.sf[1]], blobs)], out=[[dst[0], odd(0, 2)[1], dst[2]]])
    rig.sync()
    assert all(not lo.intact(g[0], g[1], 0, g[3]) for g in guards), "a refused call wrote into its destination"


def ctypes_ad(mv, ad):
    import ctypes
    return ctypes.byref(mv.AnalysisData.from_buffer_copy(bytes(ad)))


def test_super_and_finest_refusals_write_nothing(mv):
    """a 16-bit source at an odd pitch or an odd address, a Finest destination shorter than its row: MVX_E_ARG, and the destination keeps its fill"""
    frames = _cached(("refusal clip",), lambda: pl.moving_clip(206, 118, 16, 1, seed=5, noise=3))
    fill = 0x5A
    rig = Rig(mv, frames, 206, 118, 16, {}, fill, "padded", None)
    fr, ar = rig.super_frame()

    def odd(extra, residue):
        return [lo.carve(a.shape[0], a.shape[1] * 2, lo.ceil_to(a.shape[1] * 2, 256) + extra, residue, fill)[1] for a in frames[0]]
    with pytest.raises(mv.MvtoolsError, match="mvx_super_frames: src pitch must hold a row and be a multiple of the sample size"):
        rig.sup.build([odd(1, 0)], out=[fr])
    with pytest.raises(mv.MvtoolsError, match="mvx_super_frames: planes must be aligned to the sample size"):
        rig.sup.build([odd(0, 1)], out=[fr])
    short = [lo.carve(8, 64, 64, 0, fill) for _ in range(3)]
    with pytest.raises(mv.MvtoolsError, match="mvx_finest_frames: pitches must hold a row of their plane and be multiples of the sample size"):
        rig.sup.finest(rig.sf, out=[[v for _, v in short]])
    rig.sync()
    for a in ar + [a for a, _ in short]:
        assert bool((a == lo._pattern(fill, a.data_ptr(), a.numel(), a.device)).all()), "a refused call wrote into its destination"
