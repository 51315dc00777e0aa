"""GPU: BlockFPS on a float clip (mvx_blockfps_create_float) against the numpy restatement (tests/blockfps_float_ref.py, anchored to the oracle by
tests/test_blockfps_float_ref.py), sample for sample: np.array_equal on the float32 bits.

The rig is that of tests/test_gpu_compensate_float.py: the float clip is float_clip of the integer clip, the vectors are searched by Analyse on
the integer copy, never on the float samples, and the float super frames are built on the GPU and asserted to be the Super restatement's
(tests/super_float_ref.py) before the restatement runs on them.  Destinations lie inside sentinel-filled guard bands.
tests/test_blockfps_float_cases.py shows on the CPU that every masked case's masks are neither empty nor saturated; the same is asserted here
from the masks the restatement builds."""
import ctypes as C

import numpy as np
import pytest

import blockfps_float_cases as bc
import degrain_float_cases as fc
import degrain_n_cases as dc
import layouts as lo
import pipeline as pl
import super_float_ref as sf
import vector_fields

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 3
TIMES = [0, 102, 205, 51, 154, 0, 102, 205, 51, 154, 0]   # time256 of the eleven outputs of 24 -> 60 over five frames
_clips = {}


class Clip:
    """the integer clip with its super frames and both vector clips of every frame, and the float clip with its float super frames, on the
    device; the blobs also on the host"""

    def __init__(self, mv, fmt, bits, blk, w, h, delta=1):
        import torch
        self.mv, self.fmt, self.w, self.h, self.delta = mv, fmt, w, h, delta
        self.q = bc.int_clip(fmt, bits, w, h)
        self.frames = fc.float_clip(self.q, bits, seed=9)
        self.n = n = len(self.q)
        kw = dict(dc.FORMATS[fmt], **blk[1])
        self.isup = mv.Super(w, h, bits, **kw)
        isf = self.isup.build([mv.frame_to_device(f) for f in self.q])
        self.abw = mv.Analyse(self.isup, num_frames=n, isb=1, delta=delta, **blk[2])
        self.afw = mv.Analyse(self.isup, num_frames=n, isb=0, delta=delta, **blk[2])
        self.bw = self.abw.run([(isf[m], isf[m + delta] if m + delta < n else None) for m in range(n)])
        self.fw = self.afw.run([(isf[m], isf[m - delta] if m - delta >= 0 else None) for m in range(n)])
        self.fsup = mv.Super(w, h, 32, sample_float=True, **kw)
        self.src = [mv.frame_to_device(f) for f in self.frames]
        self.fsf = self.fsup.build(self.src)
        i = self.fsup.info
        self.skw = dict(sub=bc.SUB[fmt], gray=fmt == "gray", hpad=i.hpad, vpad=i.vpad, pel=i.pel, sharp=i.sharp)
        torch.cuda.synchronize()
        self.hbw = [np.asarray(b.cpu().numpy()) for b in self.bw]
        self.hfw = [np.asarray(b.cpu().numpy()) for b in self.fw]
        self.host = {}
        self.pitch = [p.stride(0) for p in self.src[0]]

    def __getitem__(self, m):
        """the GPU-built float super frame m on the host; asserted to be the Super restatement's when first fetched"""
        if m not in self.host:
            got = [self.mv.plane_to_numpy(self.fsf[m][p], self.fsup.info.plane_width[p], np.float32) for p in range(self.fsup.nplanes)]
            want, _ = sf.frame(self.frames[m], **self.skw)
            for p in range(self.fsup.nplanes):
                assert np.array_equal(got[p], want[p]), "float Super differs from its restatement: frame %d plane %d" % (m, p)
            self.host[m] = got
        return self.host[m]

    def upload(self, blobs):
        import torch
        return [torch.from_numpy(np.ascontiguousarray(b)).to("cuda") for b in blobs]


def _clip(mv, fmt, bits, blk, w, h, delta=1):
    key = (fmt, bits, blk[0], w, h, delta)
    if key not in _clips:
        _clips[key] = Clip(mv, fmt, bits, blk, w, h, delta)
    return _clips[key]


def _np(mv, t, width):
    import torch
    return mv.plane_to_numpy(t if t.dtype == torch.uint8 else t.view(torch.uint8), width, np.float32)


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


def _filter(mv, c, bkw, **kw):
    return mv.BlockFPS(c.fsup, c.abw.ad, c.afw.ad, c.n, kw.pop("pitch", c.pitch), 24, 1, num=60, den=1, sample_float=True, **dict(bkw, **kw))


def _run(mv, c, bkw, outs=None, bw=None, fw=None):
    """BlockFPS(sample_float=True) at 24 -> 60 over the output frames `outs` (all by default) in ONE call into guarded planes -> {n: planes}"""
    import torch
    b = _filter(mv, c, bkw)
    outs = list(range(b.num_frames)) if outs is None else outs
    bufs, views, rowbytes, pitch = _guarded(c, len(outs))
    assert b.is_float and b.dst_pitch == pitch == c.pitch
    b.run(outs, c.src, c.fsf, bw or c.bw, fw or c.fw, out=views)
    torch.cuda.synchronize()
    assert _guard_intact(bufs, rowbytes), "a destination plane's guard band was written"
    return b, {n: [_np(mv, views[j][p], c.frames[0][p].shape[1]) for p in range(len(c.frames[0]))] for j, n in enumerate(outs)}


def _bits(planes):
    return [np.ascontiguousarray(p).view(np.uint32) for p in planes]


def _same(got, want, what):
    assert len(got) == len(want)
    for p in range(len(want)):
        assert got[p].dtype == np.float32 and want[p].dtype == np.float32, "%s plane %d" % (what, p)
        g, w_ = _bits(got)[p], _bits(want)[p]
        if not np.array_equal(g, w_):
            ys, xs = np.nonzero(g != w_)
            pytest.fail("%s plane %d: %d samples differ, first (y=%d, x=%d) got %r want %r" % (what, p, len(ys), ys[0], xs[0], got[p][ys[0], xs[0]], want[p][ys[0], xs[0]]))


def _check(oracle, c, b, bkw, got, hbw=None, hfw=None, shares=False):
    """every output in `got` against the restatement -> (outputs that were interpolated, outputs that are not their left clip frame)"""
    ref = bc.restatement(oracle, c.abw.ad, c.afw.ad, bkw, gray=c.fmt == "gray")
    usable = moved = 0
    for n in sorted(got):
        want = bc.want_frame(ref, b.map, n, c.frames, c, hbw or c.hbw, hfw or c.hfw)
        _same(got[n], want, "output %d %s" % (n, b.map(n)))
        nl, nr, t = b.map(n)
        if ref.usable(t, 1, 1, (hfw or c.hfw)[nr] if nr < c.n else None, (hbw or c.hbw)[nl] if nr < c.n else None):
            usable += 1
            if shares and ref.mode >= 3:
                low, high = bc.mask_shares(ref)
                assert low >= bc.SHARE and high >= bc.SHARE, (n, low, high)
        moved += not np.array_equal(got[n][0], c.frames[min(nl, c.n - 1)][0])
    return usable, moved


# ------------------------------------------------------------------------------------------------ searched vectors, 24 -> 60 over five frames

@pytest.mark.parametrize("case", bc.SEARCHED, ids=bc.searched_id)
def test_24_to_60_every_output_is_the_restatements(oracle, mv, case):
    """all eleven outputs in one call: three copies (time256 0, the last of them at the clip's end) and eight interpolated frames"""
    fmt, bits, blk, w, h, mode, ml = case
    c = _clip(mv, fmt, bits, blk, w, h)
    bkw = dict(mode=mode, ml=ml)
    b, got = _run(mv, c, bkw)
    assert b.num_frames == 11 and [b.map(n)[2] for n in range(11)] == TIMES and b.map(10) == (4, 5, 0)
    usable, moved = _check(oracle, c, b, bkw, got, shares=True)
    assert usable == 8 and moved == 8
    for n in (0, 5, 10):
        assert all(np.array_equal(x, y) for x, y in zip(_bits(got[n]), _bits(c.frames[b.map(n)[0]])))


# ------------------------------------------------------------------------------------------------ all nine modes, crafted fields

def _crafted(c, recipe, bkw):
    hbw = [bc.crafted(recipe, x, c.abw.ad, 100 + m, bkw) if m + c.delta < c.n else x for m, x in enumerate(c.hbw)]
    hfw = [bc.crafted(recipe, x, c.afw.ad, 200 + m, bkw) if m - c.delta >= 0 else x for m, x in enumerate(c.hfw)]
    return hbw, hfw


@pytest.mark.parametrize("mode", range(9))
@pytest.mark.parametrize("geo", bc.MODES, ids=lambda g: bc.geo_id(*g[:5]))
def test_all_nine_modes(oracle, mv, geo, mode):
    """the occlusion profile of tests/vector_fields.py on the overlapped geometry, vectors on the limits of their legal rectangles on the other:
    masks with every value, spans of several blocks, spans cut at the grid's ends"""
    fmt, bits, blk, w, h, recipe = geo
    c = _clip(mv, fmt, bits, blk, w, h)
    bkw = dict(mode=mode, ml=bc.crafted_ml(recipe, mode))
    hbw, hfw = _crafted(c, recipe, bkw)
    b, got = _run(mv, c, bkw, outs=[1, 2, 3, 4, 5], bw=c.upload(hbw), fw=c.upload(hfw))
    usable, moved = _check(oracle, c, b, bkw, got, hbw, hfw, shares=True)
    assert usable == 4 and moved == 4
    if mode in (5, 8):  # the mask on every plane
        for n in (1, 4):
            assert all(float(p.min()) >= 0.0 and float(p.max()) <= 1.0 for p in got[n]) and len(np.unique(got[n][0])) >= 5


# ------------------------------------------------------------------------------------------------ fallbacks

@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("blk", [bc.B84, bc.B160], ids=["8/4", "16/0"])
def test_blend_at_a_scene_change_and_past_the_clips_end(oracle, mv, blk, blend):
    """one block too many above thscd1 in the backward vectors of frame 1 (tests/vector_fields.py scene_count): outputs 3 and 4 fall back; with
    delta 2, outputs 8 and 9 lie between frame 3 and a frame past the clip's end.  blend 0: the left clip frame, bit for bit; blend 1: the time
    blend of the two clip frames -- the last frame standing in for the missing one"""
    c = _clip(mv, "420", 16, blk, 96, 64)
    bkw = dict(mode=3, blend=blend)
    _, s1, s2 = vector_fields.scaled_thresholds(c.abw.ad, 400)
    hbw = list(c.hbw)
    hbw[1] = vector_fields.scene_count(c.hbw[1], c.abw.ad, 77, s1, s2 + 1, 400)
    b, got = _run(mv, c, bkw, outs=[2, 3, 4, 6], bw=c.upload(hbw))
    usable, _ = _check(oracle, c, b, bkw, got, hbw)
    assert usable == 2
    _, plain = _run(mv, c, bkw, outs=[3])
    assert not np.array_equal(plain[3][0], got[3][0])                      # (without the edit output 3 is interpolated)
    for n in (3, 4):
        same = all(np.array_equal(x, y) for x, y in zip(_bits(got[n]), _bits(c.frames[1])))
        assert same == (blend == 0)
    e = _clip(mv, "420", 16, blk, 96, 64, delta=2)
    b, got = _run(mv, e, bkw, outs=[7, 8, 9])
    assert [b.map(n) for n in (7, 8, 9)] == [(2, 4, 102), (3, 5, 25), (3, 5, 77)]
    usable, _ = _check(oracle, e, b, bkw, got)
    assert usable == 1
    for n in (8, 9):
        same = all(np.array_equal(x, y) for x, y in zip(_bits(got[n]), _bits(e.frames[3])))
        assert same == (blend == 0)
        if blend:
            t = b.map(n)[2]
            mixed = [(e.frames[3][p] * np.float32(256 - t) + e.frames[4][p] * np.float32(t)) * np.float32(1 / 256) for p in range(3)]
            _same(got[n], mixed, "the blend past the clip's end, output %d" % n)


@pytest.mark.parametrize("blk", [bc.B84, bc.B160], ids=["8/4", "16/0"])
def test_time256_0_and_256_copy_the_bits_nan_payloads_included(mv, blk):
    """jobs written by hand: time256 0 copies clip_left and 256 copies clip_right whatever the vectors say, with and without super frames;
    quiet and signalling NaNs with payloads, infinities and denormals in the clip frames arrive as they are"""
    import torch
    c = _clip(mv, "420", 16, blk, 96, 64)
    special = np.array([0x7FC12345, 0xFFC00001, 0x7F812345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000], np.uint32)
    rng = np.random.default_rng(5)
    frames = []
    for fr in c.frames[1:3]:
        planes = []
        for a in fr:
            u = np.array(a).view(np.uint32)
            idx = rng.choice(u.size, u.size // 5, replace=False)
            u.reshape(-1)[idx] = special[rng.integers(0, len(special), idx.size)]
            planes.append(u.view(np.float32))
        frames.append(planes)
    dev = [mv.frame_to_device(f) for f in frames]
    b = _filter(mv, c, dict(mode=4))
    bufs, views, rowbytes, pitch = _guarded(c, 4)
    jobs = (mv.BlockFPSJob * 4)()
    for k, (t, with_sup) in enumerate(((0, True), (256, True), (0, False), (256, False))):
        jobs[k].time256 = t
        for p in range(3):
            jobs[k].clip_left[p], jobs[k].clip_right[p], jobs[k].dst[p] = dev[0][p].data_ptr(), dev[1][p].data_ptr(), views[k][p].data_ptr()
            if with_sup:
                jobs[k].src_super[p], jobs[k].ref_super[p] = c.fsf[1][p].data_ptr(), c.fsf[2][p].data_ptr()
        if with_sup:
            jobs[k].blob_fw, jobs[k].blob_bw = c.fw[2].data_ptr(), c.bw[1].data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert mv.lib().mvx_blockfps_frames(b.h, 4, jobs, stream) == 0, mv.lib().mvx_last_error().decode()
    torch.cuda.synchronize()
    assert _guard_intact(bufs, rowbytes)
    for k, src in enumerate((0, 1, 0, 1)):
        got = [_np(mv, views[k][p], frames[0][p].shape[1]) for p in range(3)]
        assert all(np.array_equal(x, y) for x, y in zip(_bits(got), _bits(frames[src]))), "job %d" % k
        assert np.isnan(got[0]).sum() > 100


# ------------------------------------------------------------------------------------------------ crafted fields on the small sizes

@pytest.mark.parametrize("fmt,bits,blk,w,h", bc.SMALL, ids=["70x54-8/4", "70x54-16/0", "70x54-4/2-pel1", "36x36-gray-pad0"])
def test_vectors_on_the_limits_of_their_legal_rectangles_and_an_invalid_blob(oracle, mv, fmt, bits, blk, w, h):
    """every blob: a quarter of the blocks on each end of the legal rectangle in each component -- the float super frames are read up to the far
    edges of their padding, in every sub-pel plane -- with the occlusion masks such vectors give (mode 4 reads all three and both frames); the
    forward blob of frame 3 is invalid, so outputs 6 and 7 fall back"""
    c = _clip(mv, fmt, bits, blk, w, h)
    bkw = dict(mode=4, ml=bc.crafted_ml("limits", 4))
    hbw, hfw = _crafted(c, "limits", bkw)
    hfw[3] = vector_fields.invalid(hfw[3], c.afw.ad)
    xmin, xmax, ymin, ymax = vector_fields.legal_rect(c.abw.ad)
    on = np.zeros(4, bool)  # (a grid of 4 x 3 blocks need not reach every limit in one field)
    for blob, ad in [(x, c.abw.ad) for x in hbw[:4]] + [(x, c.afw.ad) for x in hfw[1:3]]:
        vx, vy, _ = pl.blob_vectors(blob, ad)
        on |= [(vx == xmin[None, :]).any(), (vx == xmax[None, :]).any(), (vy == ymin[:, None]).any(), (vy == ymax[:, None]).any()]
    assert on.all(), on
    b, got = _run(mv, c, bkw, bw=c.upload(hbw), fw=c.upload(hfw))
    usable, moved = _check(oracle, c, b, bkw, got, hbw, hfw)
    assert usable == 6 and moved == 8
    blended = [(c.frames[2][p] * np.float32(256 - 102) + c.frames[3][p] * np.float32(102)) * np.float32(1 / 256) for p in range(len(c.frames[0]))]
    _same(got[6], blended, "the invalid blob's fallback")


def test_jobs_in_one_call_are_the_jobs_run_singly(mv):
    c = _clip(mv, "420", 16, bc.B84, 96, 64)
    bkw = dict(mode=7, ml=20.0)
    _, together = _run(mv, c, bkw, outs=[4, 0, 9, 10, 2])
    for n in (4, 0, 9, 10, 2):
        _, alone = _run(mv, c, bkw, outs=[n])
        assert all(np.array_equal(x, y) for x, y in zip(_bits(together[n]), _bits(alone[n]))), n


# ------------------------------------------------------------------------------------------------ plane layouts

LAYOUTS = [("tight", "sup16"), ("plus1", "sup256"), ("offset", "sup16"), ("uv_differ", None), ("padded", None)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "%s-%s" % (l[0], l[1] or "sup"))
def test_planes_carved_out_of_arenas_of_quiet_nans_and_two_fills(oracle, mv, layout):
    """clip frames, super frames built by the GPU and destinations carved out of arenas filled with quiet NaNs and with the two byte fills, at
    tight pitches, a pitch that is an odd multiple of 4, offset planes and U != V pitches: no stray read reaches a result, nothing but samples
    is written, no input changes.  70x54: chroma cells cut by the edge and strips no block covers; outputs 1 (interpolated), 5 (a copy) and, with
    the forward blob of frame 3 invalid, 6 (the blend)"""
    import test_gpu_layouts as tl
    fmt, bits, blk, w, h = bc.SMALL[0]
    c = _clip(mv, fmt, bits, blk, w, h)
    bkw = dict(mode=7, ml=20.0)
    hfw = list(c.hfw)
    hfw[3] = vector_fields.invalid(hfw[3], c.afw.ad)
    fw = c.upload(hfw)
    outs = [1, 5, 6]
    ref = bc.restatement(oracle, c.abw.ad, c.afw.ad, bkw)
    probe = _filter(mv, c, bkw)
    want = [bc.want_frame(ref, probe.map, n, c.frames, c, c.hbw, hfw) for n in outs]
    kw = dict(dc.FORMATS[fmt], **blk[1])
    for fill in (lo.NAN_FILL,) + tuple(lo.FILLS):
        rig = tl.Rig(mv, c.frames, w, h, 32, dict(sample_float=True, **kw), fill, layout[0], layout[1])
        dst = [rig.clip_frame(layout[0], shapes=[a.shape for a in c.frames[0]]) for _ in outs]
        b = mv.BlockFPS(rig.sup, c.abw.ad, c.afw.ad, c.n, rig.src_pitch, 24, 1, num=60, den=1, sample_float=True, dst_pitch=[v.stride(0) for v in dst[0][0]], **bkw)
        rig.freeze()
        b.run(outs, rig.src, rig.sf, c.bw, fw, out=[d[0] for d in dst])
        rig.sync()
        name = "NaN fill" if not isinstance(fill, int) else "fill 0x%02x" % fill
        for k, (views, guards) in enumerate(dst):
            _same([lo.get(views[p], want[k][p].shape[1], np.float32) for p in range(3)], want[k], "%s output %d" % (name, outs[k]))
            for p, g in enumerate(guards):
                damage = lo.intact(*g[:3], g[3])
                assert not damage, "%s output %d plane %d: %s" % (name, outs[k], p, lo.describe(damage))
        assert all(bool((a == s_).all()) for (_, a), s_ in zip(rig.inputs, rig.snap)), "%s: an input was written" % name


# ------------------------------------------------------------------------------------------------ against the oracle directly

@pytest.mark.parametrize("bits,pel,akw,mode", [(16, 2, dict(blksize=16, overlap=0), 0), (8, 1, dict(blksize=8, overlap=0), 2), (16, 2, dict(blksize=8, overlap=0), 5)],
                         ids=["16bit-pel2-16/0-mode0", "8bit-pel1-8/0-mode2", "16bit-pel2-8/0-mode5"])
def test_integer_valued_super_frames_against_the_oracle(oracle, mv, bits, pel, akw, mode):
    """the oracle's level-0 super rows uploaded as an integer-valued float super frame, its blobs uploaded: modes 0 and 2 without overlap floor to
    oracle.BlockFPS's samples exactly, and mode 5 times 255 is its mask (tests/test_blockfps_float_ref.py says why)"""
    import torch
    w, h, n = 104, 70, 5  # strips right and below
    frames = dc.clip(w, h, bits, n)
    osup = oracle.Super(w, h, bits, pel=pel)
    osf = [osup.frame(f) for f in frames]
    fsup = mv.Super(w, h, 32, sample_float=True, pel=pel)
    fsf = [fsup.from_host([p[:fsup.info.plane_height[i]].astype(np.float32) for i, p in enumerate(fr)]) for fr in osf]
    abw, afw = oracle.Analyse(osup, num_frames=n, isb=1, **akw), oracle.Analyse(osup, num_frames=n, isb=0, **akw)
    hbw = [abw.frame(osf[m], osf[m + 1] if m + 1 < n else None) for m in range(n)]
    hfw = [afw.frame(osf[m], osf[m - 1] if m >= 1 else None) for m in range(n)]
    bkw = dict(mode=mode, ml=100.0)
    if mode == 5:
        hbw = [bc.crafted("limits", x, abw.ad, 100 + m, bkw) if m + 1 < n else x for m, x in enumerate(hbw)]
        hfw = [bc.crafted("limits", x, afw.ad, 200 + m, bkw) if m >= 1 else x for m, x in enumerate(hfw)]
        bkw["ml"] = bc.crafted_ml("limits", 5)
    src = [mv.frame_to_device(f) for f in fc.integer_valued(frames)]
    ob = oracle.BlockFPS(osup, abw.ad, afw.ad, n, 24, 1, num=60, den=1, **bkw)
    gb = mv.BlockFPS(fsup, abw.ad, afw.ad, n, [p.stride(0) for p in src[0]], 24, 1, num=60, den=1, sample_float=True, **bkw)
    up = lambda blobs: [torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in blobs]
    out = gb.run(list(range(ob.num_frames)), src, fsf, up(hbw), up(hfw))
    torch.cuda.synchronize()
    covW, covH = abw.ad.nBlkX * abw.ad.nBlkSizeX, abw.ad.nBlkY * abw.ad.nBlkSizeY
    for k in range(ob.num_frames):
        want = ob.frame(k, frames, osf, hbw, hfw)
        assert all(o.dtype == torch.float32 for o in out[k])
        for p in range(3):
            got = _np(mv, out[k][p], want[p].shape[1])
            cw, ch = (covW, covH) if p == 0 else (covW // 2, covH // 2)
            if mode == 5 and ob.map(k)[2]:
                assert np.array_equal(np.rint(got[:ch, :cw].astype(np.float64) * 255).astype(np.int64), want[p][:ch, :cw].astype(np.int64) >> (bits - 8)), (k, p)
                assert np.array_equal(np.floor(got[ch:]).astype(want[p].dtype), want[p][ch:])
            else:
                assert pl.first_diff(np.floor(got).astype(want[p].dtype), want[p]) == "", "output %d plane %d" % (k, p)


# ------------------------------------------------------------------------------------------------ the package, end to end

def test_torch_float32_planes_end_to_end(oracle, mv):
    """Super(sample_float=True).build -> Analyse on the integer copy -> BlockFPS(sample_float=True) on plain torch.float32 planes (rows of width
    samples, no padding): run allocates float32 planes by the destination pitch, and every output is the restatement's"""
    import torch
    w, h, n = 72, 56, 5
    q = dc.clip(w, h, 16, n)
    frames = fc.float_clip(q, 16, seed=4)
    isup = mv.Super(w, h, 16)
    isf = isup.build([mv.frame_to_device(f) for f in q])
    akw = dict(blksize=8, overlap=4)
    abw, afw = mv.Analyse(isup, num_frames=n, isb=1, **akw), mv.Analyse(isup, num_frames=n, isb=0, **akw)
    bw = abw.run([(isf[m], isf[m + 1] if m + 1 < n else None) for m in range(n)])
    fw = afw.run([(isf[m], isf[m - 1] if m >= 1 else None) for m in range(n)])
    src = [[torch.from_numpy(p).to("cuda") for p in f] for f in frames]
    assert src[0][0].dtype == torch.float32 and src[0][0].stride(0) == w
    fsup = mv.Super(w, h, bits=32, sample_float=True)
    fsf = fsup.build(src)
    bkw = dict(mode=7, ml=20.0)
    tight = [w * 4, w * 2, w * 2]
    b = mv.BlockFPS(fsup, abw.ad, afw.ad, n, tight, 24, 1, num=60, den=1, sample_float=True, **bkw)
    out = b.run(list(range(b.num_frames)), src, fsf, bw, fw)
    padded = mv.BlockFPS(fsup, abw.ad, afw.ad, n, tight, 24, 1, num=60, den=1, sample_float=True, dst_pitch=[512, 256, 256], **bkw)
    out_padded = padded.run([1, 3], src, fsf, bw, fw)
    torch.cuda.synchronize()
    assert b.is_float and b.dst_pitch == tight and len(out) == 11
    assert all(o.dtype == torch.float32 and o.shape == s.shape for fr in out for o, s in zip(fr, src[0]))
    assert all(o.dtype == torch.float32 and o.shape == (s.shape[0], 512 // 4 if p == 0 else 256 // 4) for fr in out_padded for p, (o, s) in enumerate(zip(fr, src[0])))
    sup_np = [[mv.plane_to_numpy(fsf[m][p], fsup.info.plane_width[p], np.float32) for p in range(3)] for m in range(n)]
    for m in range(n):
        want, _ = sf.frame(frames[m])
        assert all(np.array_equal(sup_np[m][p], want[p]) for p in range(3))
    hbw, hfw = [x.cpu().numpy() for x in bw], [x.cpu().numpy() for x in fw]
    ref = bc.restatement(oracle, abw.ad, afw.ad, bkw)
    for k in range(11):
        want = bc.want_frame(ref, b.map, k, frames, sup_np, hbw, hfw)
        _same([o.cpu().numpy() for o in out[k]], want, "output %d" % k)
        if k in (1, 3):
            _same([o[:, :s.shape[1]].cpu().numpy() for o, s in zip(out_padded[[1, 3].index(k)], src[0])], want, "padded output %d" % k)
    assert all(torch.equal(a, b_) for a, b_ in zip(out[5], src[2]))                                   # time256 0: the clip frame
    with pytest.raises(mv.MvtoolsError, match="BlockFPS: float super clips are not supported."):
        mv.BlockFPS(fsup, abw.ad, afw.ad, n, tight, 24, 1)
