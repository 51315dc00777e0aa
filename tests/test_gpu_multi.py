"""GPU: AnalyseN, CompensateN and DegrainN on a multi blob through the C ABI, byte for byte against the entry points they are made of.

Every field of a multi blob is held to the mv.Analyse run it stands for (which tests/test_gpu_parity.py pins to the oracle), every compensated
frame to mv.Compensate on the same (source, reference, field), the centre to the clip frame, and DegrainN on a multi blob to DegrainN on the
list of blobs.  Every frame of the clip is a job, so both clip ends -- references outside the clip -- are in every case.
tests/test_multi_cases.py shows on the CPU that at the cases' thsad most far blocks are compensated and some are not; the same is asserted
here from the searched fields."""
import numpy as np
import pytest

import degrain_n_cases as dc
import multi_cases as mc
import pipeline as pl
import vector_fields

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 3
_clips = {}


class Clip:
    """a clip on the device, its super frames, the multi blob of every frame (searched in ONE AnalyseN call over pad bytes set to a sentinel),
    and on demand the blobs of the 2 * radius Analyse objects the fields stand for"""

    def __init__(self, mv, fmt, bits, blk, radius, w, h, extra):
        import torch
        self.mv, self.fmt, self.radius = mv, fmt, radius
        self.frames = dc.clip(w, h, bits, mc.nframes(radius), fmt)
        self.n = len(self.frames)
        self.sup = mv.Super(w, h, bits, **dict(dc.FORMATS[fmt], **blk[1]))
        self.src = [mv.frame_to_device(f) for f in self.frames]
        self.sf = self.sup.build(self.src)
        self.akw = dict(blk[2], **extra)
        self.an = mv.AnalyseN(self.sup, radius, num_frames=self.n, **self.akw)
        self.nrefs = [mv.multi_refs(n, radius, self.n) for n in range(self.n)]
        self.refs = [[self.sf[m] if m is not None else None for m in row] for row in self.nrefs]
        self.multi = self.an.alloc_blobs(self.n)
        for b in self.multi:
            b.fill_(SENTINEL)
        self.an.run([(self.sf[n], self.refs[n]) for n in range(self.n)], blobs=self.multi)
        torch.cuda.synchronize()
        self._singles = None

    def singles(self):
        """[r][n]: what the Analyse of field r writes for frame n (over the same sentinel), and that object's analysis data"""
        if self._singles is None:
            blobs, ads = [], []
            for r in range(2 * self.radius):
                isb, d = mc.field_of(r)
                one = self.mv.Analyse(self.sup, num_frames=self.n, isb=isb, delta=d, **self.akw)
                mine = one.alloc_blobs(self.n)
                for b in mine:
                    b.fill_(SENTINEL)
                blobs.append(one.run([(self.sf[n], self.refs[n][r]) for n in range(self.n)], blobs=mine))
                ads.append(one.ad)
            self._singles = (blobs, ads)
        return self._singles

    def planes(self, frame):
        return [self.mv.plane_to_numpy(frame[p], self.frames[0][p].shape[1], self.frames[0][p].dtype) for p in range(len(self.frames[0]))]


def _clip(mv, fmt, bits, blk, radius, w=mc.W, h=mc.H, **extra):
    key = (fmt, bits, blk[0], radius, w, h, tuple(sorted(extra.items())))
    if key not in _clips:
        _clips[key] = Clip(mv, fmt, bits, blk, radius, w, h, extra)
    return _clips[key]


def _guarded(c, count):
    """count frames whose planes lie inside sentinel-filled buffers: GUARD rows above and below, the pitch padding to the right"""
    import torch
    i = c.sup.info
    hs = [i.height] + [i.height // i.yRatioUV] * 2
    ws = [i.width] + [i.width // i.xRatioUV] * 2
    pitch = [((ws[p] * c.sup.bps + 255) // 256) * 256 for p in range(c.sup.nplanes)]
    bufs = [[torch.full((hs[p] + 2 * GUARD, pitch[p]), SENTINEL, dtype=torch.uint8, device="cuda") for p in range(c.sup.nplanes)] for _ in range(count)]
    views = [[b[p][GUARD:GUARD + hs[p]] for p in range(c.sup.nplanes)] for b in bufs]
    return bufs, views, [ws[p] * c.sup.bps for p in range(c.sup.nplanes)], pitch


def _guard_intact(bufs, rowbytes):
    for fr in bufs:
        for p, b in enumerate(fr):
            a = b.cpu().numpy()
            if not ((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all() and (a[:, rowbytes[p]:] == SENTINEL).all()):
                return False
    return True


# ------------------------------------------------------------------------------------------------ AnalyseN

ANALYSE_CASES = [(c, {}) for c in mc.cases()] + [(("420", 8, mc.B84, 3), dict(search=3)), (("420", 8, mc.B84, 2), dict(divide=1)),
                                                  (("420", 16, mc.B160, 2), dict(search=3, searchparam=4, chroma=0))]


@pytest.mark.parametrize("case,extra", ANALYSE_CASES, ids=lambda v: mc.case_id(v) if isinstance(v, tuple) else ",".join("%s=%s" % kv for kv in v.items()))
def test_every_field_is_the_blob_of_its_analyse(mv, case, extra):
    fmt, bits, blk, radius = case
    c = _clip(mv, fmt, bits, blk, radius, **extra)
    blobs, ads = c.singles()
    size, stride = c.an.field_size, c.an.field_stride
    assert c.multi[0].numel() == c.an.blob_size == 2 * radius * stride
    invalid = 0
    for n in range(c.n):
        whole = c.multi[n].cpu().numpy()
        views = c.an.fields(c.multi[n])
        for r in range(2 * radius):
            want = blobs[r][n].cpu().numpy()
            assert want.size == size
            assert np.array_equal(views[r].cpu().numpy(), want), "frame %d field %d" % (n, r)
            assert np.array_equal(whole[r * stride:r * stride + size], want)
            assert (whole[r * stride + size:(r + 1) * stride] == SENTINEL).all(), "pad bytes behind field %d of frame %d" % (r, n)
            valid = int(want[4:8].view(np.int32)[0])
            assert valid == (c.nrefs[n][r] is not None)
            invalid += not valid
    assert invalid == radius * (radius + 1)  # (each clip end: radius + (radius - 1) + ... + 1 references outside the clip)
    for r in range(2 * radius):
        assert bytes(c.an.ad(r)) == bytes(ads[r])
    if not extra.get("divide"):  # the searched vectors follow the motion: not an all-zero field
        vx, _, _ = pl.blob_vectors(blobs[0][radius + 1].cpu().numpy(), ads[0])
        assert np.count_nonzero(vx) > vx.size // 2


def test_the_cases_leave_pad_bytes_to_check(mv):
    sup = mv.Super(mc.W, mc.H, 8, pel=2)
    an = mv.AnalyseN(sup, 2, blksize=8, overlap=4)
    assert 0 < an.field_size < an.field_stride


# ------------------------------------------------------------------------------------------------ CompensateN

def _compensate_case(mv, c, ckw, multi=None, frames=None):
    """CompensateN over `frames` of the clip (all by default) in one call into guarded planes, and Compensate on every (source, reference,
    field) of them -> [(n, k, got planes, want planes or None for the centre)]"""
    import torch
    tr = c.radius
    frames = list(range(c.n)) if frames is None else frames
    multi = multi or c.multi
    cn = mv.CompensateN(tr, c.sup, c.an.ad(0), **ckw)
    no = 2 * tr + 1
    bufs, views, rowbytes, pitch = _guarded(c, no * len(frames))
    assert cn.dst_pitch == pitch
    out = [views[j * no:(j + 1) * no] for j in range(len(frames))]
    cn.run([(c.sf[n], c.refs[n], multi[n]) for n in frames], out=out)
    want = {}
    for k in range(no):
        off, field = cn.map(k)
        if field < 0:
            continue
        comp = mv.Compensate(c.sup, c.an.ad(field), **ckw)
        res = comp.run([(c.sf[n], c.refs[n][field], c.an.fields(multi[n])[field]) for n in frames])
        for j, n in enumerate(frames):
            want[(n, k)] = res[j]
    torch.cuda.synchronize()
    assert _guard_intact(bufs, rowbytes), "a destination plane's guard band was written"
    return [(n, k, c.planes(out[j][k]), c.planes(want[(n, k)]) if (n, k) in want else None) for j, n in enumerate(frames) for k in range(no)]


def _check_outputs(c, results):
    tr = c.radius
    moved = 0
    for n, k, got, want in results:
        if want is None:
            assert k == tr
            want = c.frames[n]
        for p in range(len(want)):
            assert pl.first_diff(got[p], want[p]) == "", "frame %d output %d plane %d" % (n, k, p)
        if k != tr and 0 <= n + k - tr < c.n:
            moved += not np.array_equal(got[0], c.frames[n][0])
    return moved


@pytest.mark.parametrize("case", mc.cases(), ids=mc.case_id)
def test_every_output_is_compensates_and_the_centre_is_the_clip(mv, case):
    fmt, bits, blk, radius = case
    c = _clip(mv, fmt, bits, blk, radius)
    # what tests/test_multi_cases.py shows through the oracle, from the searched fields of the middle frame
    fields = c.an.fields(c.multi[radius + 1])
    sads = [pl.blob_vectors(f.cpu().numpy(), c.an.ad(r))[2] for r, f in enumerate(fields)]
    used, unused = mc.far_shares(sads, c.an.ad(0), mc.THSAD, radius)
    assert used >= mc.USED and unused >= mc.UNUSED
    moved = _check_outputs(c, _compensate_case(mv, c, dict(thsad=mc.THSAD)))
    assert moved >= radius  # (compensated frames are not copies of the source)


@pytest.mark.parametrize("blk", [mc.B84, mc.B160], ids=lambda b: b[0])
def test_time_50(mv, blk):
    c = _clip(mv, "420", 8, blk, 2)
    full = _compensate_case(mv, c, dict(thsad=mc.THSAD), frames=[3])
    half = _compensate_case(mv, c, dict(thsad=mc.THSAD, time=50.0), frames=[3])
    _check_outputs(c, half)
    assert any(not np.array_equal(a[2][0], b[2][0]) for a, b in zip(full, half))


@pytest.mark.parametrize("scbehavior", [0, 1])
@pytest.mark.parametrize("fmt,bits,blk", [("420", 8, mc.B84), ("420", 16, mc.B160)], ids=["8bit-p2", "16bit-p1"])
def test_a_scene_change_in_one_field(mv, fmt, bits, blk, scbehavior):
    """field 3 (forward, distance 2) of the middle frame carries one block too many above thscd1 (tests/vector_fields.py scene_count): that
    output is the reference frame at scbehavior 0 and the source at 1, and the other outputs are not touched by it"""
    import torch
    tr, n, field = 3, 4, 3
    c = _clip(mv, fmt, bits, blk, tr)
    ad = c.an.ad(field)
    th, s1, s2 = vector_fields.scaled_thresholds(ad, mc.THSAD)
    multi = list(c.multi)
    multi[n] = c.multi[n].clone()
    view = c.an.fields(multi[n])[field]
    view.copy_(torch.from_numpy(vector_fields.scene_count(view.cpu().numpy(), ad, 77, s1, s2 + 1, th)).to(view.device))
    results = _compensate_case(mv, c, dict(thsad=mc.THSAD, scbehavior=scbehavior), multi=multi, frames=[n, 0])
    _check_outputs(c, results)
    k = tr - 2
    got = [g for m, kk, g, _ in results if (m, kk) == (n, k)][0]
    want = c.frames[n] if scbehavior else c.frames[n - 2]
    for p in range(len(want)):
        assert pl.first_diff(got[p], want[p]) == "", "plane %d" % p
    assert not np.array_equal(got[0], c.planes(mv.CompensateN(tr, c.sup, c.an.ad(0), thsad=mc.THSAD, scbehavior=scbehavior).run(
        [(c.sf[n], c.refs[n], c.multi[n])])[0][k])[0])  # (without the edit that output is a compensated frame)


@pytest.mark.parametrize("bits,blk", [(8, mc.B160), (8, mc.B84), (16, mc.B160)], ids=["8bit-p1", "8bit-p2", "16bit-p1"])
def test_strips_no_block_covers_and_cells_that_leave_the_frame(mv, bits, blk):
    """104x70: blocks of 16 cover 96x64 and leave strips right and below, and the last 16-sample (chroma 8-sample) cell of a row is cut by the
    frame's edge; blocks of 8 stepping by 4 cover the width and leave two rows"""
    c = _clip(mv, "420", bits, blk, 2, w=104, h=70)
    ad = c.an.ad(0)
    assert (ad.nBlkX * (ad.nBlkSizeX - ad.nOverlapX) + ad.nOverlapX, ad.nBlkY * (ad.nBlkSizeY - ad.nOverlapY) + ad.nOverlapY) != (104, 70)
    for scb in (0, 1):
        _check_outputs(c, _compensate_case(mv, c, dict(thsad=mc.THSAD, scbehavior=scb)))


def test_jobs_in_one_call_are_the_jobs_run_singly(mv):
    c = _clip(mv, "420", 8, mc.B84, 3)
    cn = mv.CompensateN(3, c.sup, c.an.ad(0), thsad=mc.THSAD)
    jobs = [(c.sf[n], c.refs[n], c.multi[n]) for n in (4, 0, 8, 5)]
    together = [[c.planes(fr) for fr in job] for job in cn.run(jobs)]
    for j, job in enumerate(jobs):
        alone = [c.planes(fr) for fr in cn.run([job])[0]]
        for k in range(7):
            for p in range(3):
                assert np.array_equal(together[j][k][p], alone[k][p]), (j, k, p)
    assert not np.array_equal(together[0][0][0], together[3][0][0])


# ------------------------------------------------------------------------------------------------ DegrainN on a multi blob

@pytest.mark.parametrize("radius", mc.RADII)
@pytest.mark.parametrize("fmt,bits,blk", [("420", 8, mc.B84), ("420", 16, mc.B160), ("gray", 8, mc.B160)], ids=["420-8bit-p2", "420-16bit-p1", "gray-8bit-p1"])
def test_degrain_n_takes_a_multi_blob_for_the_list_of_blobs(mv, fmt, bits, blk, radius):
    c = _clip(mv, fmt, bits, blk, radius)
    pitch = [p.stride(0) for p in c.src[0]]
    dg = mv.DegrainN(radius, c.sup, c.an.ad(0), pitch)
    frames = [radius + 1, 0, c.n - 1]
    blobs, _ = c.singles()
    got = dg.run([(c.src[n], c.refs[n], c.multi[n]) for n in frames])
    want = dg.run([(c.src[n], c.refs[n], [blobs[r][n] for r in range(2 * radius)]) for n in frames])
    views = dg.run([(c.src[n], c.refs[n], c.an.fields(c.multi[n])) for n in frames])
    for j, n in enumerate(frames):
        g, w, v = c.planes(got[j]), c.planes(want[j]), c.planes(views[j])
        for p in range(len(w)):
            assert pl.first_diff(g[p], w[p]) == "" and pl.first_diff(v[p], w[p]) == "", "frame %d plane %d" % (n, p)
        assert not np.array_equal(w[0], c.frames[n][0])
    with pytest.raises(ValueError):
        dg.run([(c.src[0], c.refs[0], c.multi[0][:-1])])
