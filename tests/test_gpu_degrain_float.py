"""GPU: DegrainN on a float clip (mvx_degrain_n_create_float) against the numpy restatement (tests/degrain_float_ref.py, anchored to the integer
restatement by tests/test_degrain_float_ref.py), sample for sample (np.array_equal on float32, no NaN anywhere).

The float clip is the suite's moving texture plus noise, so weights differ per block; the vectors are searched by AnalyseN on its quantised copy
(round(x * 65535), or the 8-bit copy), never on the float samples.  The restatement runs on the GPU-built float super frames, and every pipe
first asserts that those frames are the Super restatement's (tests/super_float_ref.py), so a Degrain failure is not a Super failure in disguise.

    A  70 x 54   4:2:0 chroma is 35 x 27: partial cells, strips no block covers
    B  140 x 38  the padded luma crosses a tile seam of the float level-0 kernel
    C  36 x 36   Gray, pad 0"""
import numpy as np
import pytest

import degrain_float_cases as fc
import degrain_n_cases as dc
import pipeline as pl
import super_float_ref as sf
import vector_fields

pytestmark = pytest.mark.gpu

SIZES = {"A": (70, 54), "B": (140, 38), "C": (36, 36)}
SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "gray": (1, 1)}
B168, B84, B42 = dict(blksize=16, overlap=8), dict(blksize=8, overlap=4), dict(blksize=4, overlap=2)
B80, B160, B1684 = dict(blksize=8, overlap=0), dict(blksize=16, overlap=0), dict(blksize=16, blksizev=8, overlap=8, overlapv=4)
PAD0 = dict(hpad=0, vpad=0)

_pipes = {}


class Pipe:
    """the integer clip with its super frames (for the search) and the float clip with its float super frames (for the filter), on the device"""

    def __init__(self, mv, size, fmt, bits, skw, n, noise=3):
        w, h = SIZES[size] if isinstance(size, str) else size
        self.mv, self.fmt, self.n, self.bits, self.w, self.h = mv, fmt, n, bits, w, h
        self.q = dc.clip(w, h, bits, n, fmt, noise=noise)
        self.frames = fc.float_clip(self.q, bits, seed=9)
        kw = dict(dc.FORMATS[fmt], **skw)
        self.isup = mv.Super(w, h, bits, **kw)
        self.isf = self.isup.build([mv.frame_to_device(f) for f in self.q])
        self.fsup = mv.Super(w, h, 32, sample_float=True, **kw)
        self.src = [mv.frame_to_device(f) for f in self.frames]
        self.fsf = self.fsup.build(self.src)
        self.skw = dict(sub=SUB[fmt], gray=fmt == "gray", hpad=self.fsup.info.hpad, vpad=self.fsup.info.vpad, pel=self.fsup.info.pel, sharp=self.fsup.info.sharp)
        self.host, self.searches = {}, {}

    def sup_np(self, m):
        """the GPU-built float super frame m on the host; asserted to be the Super restatement's when first fetched"""
        if m not in self.host:
            import torch
            torch.cuda.synchronize()
            got = [self.mv.plane_to_numpy(self.fsf[m][p], self.fsup.info.plane_width[p], np.float32) for p in range(self.fsup.nplanes)]
            want, _ = sf.frame(self.frames[m], **self.skw)
            for p in range(self.fsup.nplanes):
                assert np.array_equal(got[p], want[p]), "float Super differs from its restatement: frame %d plane %d" % (m, p)
            self.host[m] = got
        return self.host[m]

    def search(self, target, radius, akw):
        """AnalyseN on the integer copy -> (analysis data of field 0, reference frame numbers or None, the multi blob, its fields)"""
        key = (target, radius, tuple(sorted(akw.items())))
        if key not in self.searches:
            an = self.mv.AnalyseN(self.isup, radius, num_frames=self.n, **akw)
            nrefs = self.mv.multi_refs(target, radius, self.n)
            mb = an.run([(self.isf[target], [self.isf[m] if m is not None else None for m in nrefs])])[0]
            self.searches[key] = (an.ad(0), nrefs, mb, an.fields(mb))
        return self.searches[key]

    def pitch(self):
        return [p.stride(0) for p in self.src[0]]

    def refs(self, nrefs):
        return [self.fsf[m] if m is not None else None for m in nrefs]

    def planes(self, out):
        import torch
        torch.cuda.synchronize()
        return [self.mv.plane_to_numpy(out[p], self.frames[0][p].shape[1], np.float32) for p in range(len(self.frames[0]))]


def _pipe(mv, size, fmt, bits, skw, n, **kw):
    key = (size, fmt, bits, tuple(sorted(skw.items())), n, tuple(sorted(kw.items())))
    if key not in _pipes:
        _pipes[key] = Pipe(mv, size, fmt, bits, skw, n, **kw)
    return _pipes[key]


def _want(oracle, pipe, ad, radius, dkw, target, nrefs, blobs, info):
    """the restatement's planes for one job (blobs: host arrays) and the restatement"""
    ref = fc.restatement(oracle, radius, ad, info["thsad_d"], info["thsadc_d"], dkw, gray=pipe.fmt == "gray")
    want = ref.frame(pipe.frames[target], [pipe.sup_np(m) if m is not None else None for m in nrefs], blobs)
    return want, ref


def _same(got, want, what):
    assert len(got) == len(want)
    for p in range(len(want)):
        assert got[p].dtype == np.float32 and want[p].dtype == np.float32 and not np.isnan(got[p]).any()
        assert pl.first_diff(got[p], want[p]) == "", "%s plane %d" % (what, p)


def _host(blobs):
    return [np.asarray(b.cpu().numpy()) for b in blobs]


# ------------------------------------------------------------------------------------------------ searched vectors

def _cases():
    c = []
    for akw in (B168, B84, B42, B80, B160, B1684):           # the cell widths 8 / 4 / 2 / 1 and blocks side by side, radius 3, pel 2
        c.append(("A", "420", 16, {}, akw, 3, {}))
    for akw in (B168, B84, B42):                             # lists of 2 and of up to 14 entries
        c += [("A", "420", 16, {}, akw, 1, {}), ("A", "420", 16, {}, akw, 7, dict(thsad=1200))]
    for pel in (1, 4):
        for akw in (B168, B84, B80):
            c.append(("A", "420", 16, dict(pel=pel), akw, 3, {}))
    c += [("A", "422", 16, {}, B168, 3, {}), ("A", "444", 16, {}, B84, 3, {}), ("A", "gray", 16, {}, B168, 1, {}), ("A", "444", 16, dict(pel=4), B42, 1, {})]
    c += [("B", "420", 16, {}, B84, 3, {}), ("B", "420", 16, dict(hpad=8, vpad=4), B168, 1, {})]
    c += [("C", "gray", 16, PAD0, B84, 3, {}), ("C", "gray", 16, dict(PAD0, pel=1), B42, 1, {})]
    for akw in (B168, B84, B42, B80):                        # the search on the 8-bit copy
        c.append(("A", "420", 8, {}, akw, 3, {}))
    c += [("A", "420", 16, {}, B84, 7, dict(thsad=1600, thsad2=400)), ("A", "420", 16, {}, B168, 3, dict(plane=0)), ("A", "420", 16, {}, B168, 3, dict(plane=3)),
          ("A", "420", 16, {}, B84, 3, dict(limit=10, limitc=5)), ("A", "420", 16, {}, B168, 1, dict(limit=1, limitc=0)), ("A", "420", 8, {}, B84, 3, dict(limit=10, limitc=5)),
          ("A", "420", 16, {}, B80, 3, dict(limit=2))]
    return c


CASES = _cases()


def _id(c):
    size, fmt, bits, skw, akw, radius, dkw = c
    return "%s-%s-%dbit-r%d-%s" % (size, fmt, bits, radius, ",".join("%s=%s" % kv for d in (skw, akw, dkw) for kv in sorted(d.items())))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_plane_is_the_restatements(oracle, mv, case):
    size, fmt, bits, skw, akw, radius, dkw = case
    n = 2 * radius + 1
    pipe = _pipe(mv, size, fmt, bits, skw, n)
    ad, nrefs, mb, fields = pipe.search(radius, radius, akw)
    dg = mv.DegrainN(radius, pipe.fsup, ad, pipe.pitch(), **dkw)
    assert dg.is_float and dg.out_bits == 32
    got = pipe.planes(dg.run([(pipe.src[radius], pipe.refs(nrefs), mb)])[0])   # the multi blob itself
    want, ref = _want(oracle, pipe, ad, radius, dkw, radius, nrefs, _host(fields), dg.info())
    w = ref.plan[0][1]
    assert np.count_nonzero(w) and len(np.unique(w[w > 0])) > 3, "the weights do not differ per block"
    _same(got, want, _id(case))
    if dkw.get("plane", 4) != 3:
        assert not np.array_equal(got[0], pipe.frames[radius][0])
    again = pipe.planes(dg.run([(pipe.src[radius], pipe.refs(nrefs), list(fields))])[0])  # ... and the list of its fields
    _same(again, want, "list of blobs")


@pytest.mark.parametrize("akw", [B168, B84], ids=["16/8", "8/4"])
@pytest.mark.parametrize("target", [0, 6], ids=["first", "last"])
def test_clip_ends(oracle, mv, target, akw):
    """references outside the clip (NULL planes, invalid blobs); two jobs in one call are the two run singly"""
    pipe = _pipe(mv, "A", "420", 16, {}, 7)
    ad, nrefs, mb, fields = pipe.search(target, 3, akw)
    assert [m is None for m in nrefs] == [bool(r % 2) == (target == 0) for r in range(6)]
    ad2, nrefs2, mb2, fields2 = pipe.search(3, 3, akw)
    dg = mv.DegrainN(3, pipe.fsup, ad, pipe.pitch())
    outs = dg.run([(pipe.src[target], pipe.refs(nrefs), mb), (pipe.src[3], pipe.refs(nrefs2), mb2)])
    want, ref = _want(oracle, pipe, ad, 3, {}, target, nrefs, _host(fields), dg.info())
    assert not np.any(ref.plan[0][1][:, [r for r in range(6) if nrefs[r] is None]]) and np.count_nonzero(ref.plan[0][1])
    _same(pipe.planes(outs[0]), want, "end")
    want2, _ = _want(oracle, pipe, ad2, 3, {}, 3, nrefs2, _host(fields2), dg.info())
    _same(pipe.planes(outs[1]), want2, "middle")


@pytest.mark.parametrize("akw", [B168, B80], ids=["16/8", "8/0"])
def test_a_job_without_a_usable_reference_keeps_its_source_bit_for_bit(oracle, mv, akw):
    """thscd1 so low that every blob counts as a scene change; every reference outside the clip; an invalid blob"""
    import torch
    pipe = _pipe(mv, "A", "420", 16, {}, 7)
    ad, nrefs, mb, fields = pipe.search(3, 3, akw)
    bits = lambda planes: [p.view(np.uint32) for p in planes]
    src = bits(pipe.frames[3])
    dg = mv.DegrainN(3, pipe.fsup, ad, pipe.pitch(), thscd1=1, thscd2=0)
    got = pipe.planes(dg.run([(pipe.src[3], pipe.refs(nrefs), mb)])[0])
    want, ref = _want(oracle, pipe, ad, 3, dict(thscd1=1, thscd2=0), 3, nrefs, _host(fields), dg.info())
    assert not np.count_nonzero(ref.plan[0][1])
    for p in range(3):
        assert np.array_equal(bits(got)[p], src[p]) and np.array_equal(bits(want)[p], src[p]), p
    dg = mv.DegrainN(3, pipe.fsup, ad, pipe.pitch())
    got = pipe.planes(dg.run([(pipe.src[3], [None] * 6, [None] * 6)])[0])
    assert all(np.array_equal(bits(got)[p], src[p]) for p in range(3))
    dead = [torch.from_numpy(vector_fields.invalid(b, ad)).to(mb.device) for b in _host(fields)]
    got = pipe.planes(dg.run([(pipe.src[3], pipe.refs(nrefs), dead)])[0])
    assert all(np.array_equal(bits(got)[p], src[p]) for p in range(3))
    # one invalid blob among valid ones: that reference alone drops out
    mixed = list(fields)
    mixed[1] = dead[1]
    got = pipe.planes(dg.run([(pipe.src[3], pipe.refs(nrefs), mixed)])[0])
    want, ref = _want(oracle, pipe, ad, 3, {}, 3, nrefs, _host(mixed), dg.info())
    assert not np.any(ref.plan[0][1][:, 1]) and np.count_nonzero(ref.plan[0][1])
    _same(got, want, "one invalid blob")


# ------------------------------------------------------------------------------------------------ crafted fields

@pytest.mark.parametrize("size,fmt,skw,akw", [("A", "420", dict(pel=1), B168), ("A", "420", {}, B84), ("A", "420", dict(pel=4), B42), ("A", "444", dict(pel=4), B168),
                                              ("B", "420", dict(hpad=8, vpad=4), B84), ("C", "gray", PAD0, B84), ("A", "422", {}, B160)],
                         ids=["A-pel1-16/8", "A-pel2-8/4", "A-pel4-4/2", "A-444-pel4-16/8", "B-pad8x4-8/4", "C-gray-pad0-8/4", "A-422-16/0"])
def test_vectors_on_the_limits_of_their_legal_rectangles(oracle, mv, size, fmt, skw, akw):
    """tests/vector_fields.py `limits`: a quarter of the blocks on each end of the legal rectangle in each component, small SADs: the float super
    frame is read up to the far edges of its padding, in every sub-pel plane"""
    import torch
    pipe = _pipe(mv, size, fmt, 16, skw, 3)
    ad, nrefs, mb, fields = pipe.search(1, 1, akw)
    crafted = [vector_fields.limits(b, ad, 70 + r) for r, b in enumerate(_host(fields))]
    xmin, xmax, ymin, ymax = vector_fields.legal_rect(ad)
    vx, vy, _ = pl.blob_vectors(crafted[0], ad)
    assert (vx == xmin[None, :]).any() and (vx == xmax[None, :]).any() and (vy == ymin[:, None]).any() and (vy == ymax[:, None]).any()
    dg = mv.DegrainN(1, pipe.fsup, ad, pipe.pitch())
    got = pipe.planes(dg.run([(pipe.src[1], pipe.refs(nrefs), [torch.from_numpy(b).to(mb.device) for b in crafted])])[0])
    want, ref = _want(oracle, pipe, ad, 1, {}, 1, nrefs, crafted, dg.info())
    assert np.all(ref.plan[0][1] > 0)
    _same(got, want, "limits")


def test_a_field_scaled_by_scale_vect(oracle, mv):
    """an 8-bit search at half size, ScaleVect to the full-size geometry (its target is an integer super clip of that geometry: it refuses a float
    one), the float clip filtered at full size"""
    w, h = 192, 128
    pipe = _pipe(mv, (w, h), "420", 16, dict(hpad=32, vpad=32), 3)
    small = [[(p.astype(np.uint32).reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2).sum(axis=(1, 3)) // (4 * 257)).astype(np.uint8) for p in f] for f in pipe.q]
    ssup = mv.Super(w // 2, h // 2, 8)
    ssf = ssup.build([mv.frame_to_device(f) for f in small])
    blobs, ad_small = [], None
    for isb, m in ((1, 2), (0, 0)):
        an = mv.Analyse(ssup, isb=isb, **B84)
        blobs.append(an.run([(ssf[1], ssf[m])])[0])
        ad_small = ad_small or an.ad
    with pytest.raises(mv.MvtoolsError, match="ScaleVect: float super clips are not supported."):
        mv.ScaleVect(ad_small, pipe.fsup, 2)
    sv = mv.ScaleVect(ad_small, pipe.isup, 2)
    scaled = sv.run(blobs)
    assert (sv.ad.nBlkSizeX, sv.ad.nOverlapX, sv.ad.bitsPerSample) == (16, 8, 16)
    dg = mv.DegrainN(1, pipe.fsup, sv.ad, pipe.pitch(), thsad=1600)
    got = pipe.planes(dg.run([(pipe.src[1], [pipe.fsf[2], pipe.fsf[0]], scaled)])[0])
    want, ref = _want(oracle, pipe, sv.ad, 1, dict(thsad=1600), 1, [2, 0], _host(scaled), dg.info())
    assert np.count_nonzero(ref.plan[0][1])
    _same(got, want, "scaled field")


# ------------------------------------------------------------------------------------------------ the package, end to end

def test_torch_float32_planes_end_to_end(oracle, mv):
    """Super(sample_float=True).build and DegrainN.run on plain torch.float32 planes (rows of width samples, no padding)"""
    import torch
    w, h, n = SIZES["A"][0] + 2, SIZES["A"][1] + 2, 3     # 72 x 56: rows of 288 and 144 bytes
    q = dc.clip(w, h, 16, n)
    frames = fc.float_clip(q, 16, seed=4)
    isup = mv.Super(w, h, 16)
    isf = isup.build([mv.frame_to_device(f) for f in q])
    an = mv.AnalyseN(isup, 1, num_frames=n, **B84)
    mb = an.run([(isf[1], [isf[2], isf[0]])])[0]
    src = [[torch.from_numpy(p).to("cuda") for p in f] for f in frames]
    assert src[0][0].dtype == torch.float32 and src[0][0].stride(0) == w
    fsup = mv.Super(w, h, bits=32, sample_float=True)
    fsf = fsup.build(src)
    dg = mv.DegrainN(1, fsup, an.ad(0), [w * 4, w * 2, w * 2], limit=20)
    out = dg.run([(src[1], [fsf[2], fsf[0]], mb)])[0]
    torch.cuda.synchronize()
    assert all(o.dtype == torch.float32 and o.shape == s.shape for o, s in zip(out, src[1]))
    sup_np = [[mv.plane_to_numpy(fr[p], fsup.info.plane_width[p], np.float32) for p in range(3)] for fr in (fsf[2], fsf[0])]
    for fr, m in zip(sup_np, (2, 0)):
        want, _ = sf.frame(frames[m])
        assert all(np.array_equal(fr[p], want[p]) for p in range(3))
    ref = fc.restatement(oracle, 1, an.ad(0), dg.info()["thsad_d"], dg.info()["thsadc_d"], dict(limit=20))
    want = ref.frame(frames[1], sup_np, _host(an.fields(mb)))
    _same([o.cpu().numpy() for o in out], want, "end to end")
    with pytest.raises(mv.MvtoolsError, match="DegrainN: float super clips are not supported."):
        mv.DegrainN(1, fsup, an.ad(0), [w * 4, w * 2, w * 2], out16=True)
