"""GPU: mv.DegrainN (temporal radius 1..24, thresholds per distance) through the C ABI, byte for byte.

Up to radius 6 it is held to mv.Degrain, which the oracle pins (tests/test_gpu_parity.py): DegrainN always runs its own kernels, so this
compares the new code with the old on the same vectors.  Beyond 6 it is held to the numpy restatement (tests/degrain_n_ref.py), which
tests/test_degrain_n_ref.py holds to the oracle at radii 1, 2, 3 and 6; the vectors come from the GPU search at delta 1..radius, and the
thresholds per distance from info(), whose table tests/test_degrain_n_host.py checks.  tests/test_degrain_n_cases.py shows on the CPU that
in each of those cases most far references carry a weight and some carry none; the same is asserted here from the restatement's plan."""
import numpy as np
import pytest

import degrain_n_cases as dc
import pipeline as pl
import vector_fields

pytestmark = pytest.mark.gpu

_pipes, _jobs = {}, {}


class Pipe:
    """a clip on the device with its super frames; host copies of the super frames on demand"""

    def __init__(self, mv, frames, w, h, bits, fmt, skw):
        self.mv, self.frames, self.fmt = mv, frames, fmt
        self.sup = mv.Super(w, h, bits, **dict(dc.FORMATS[fmt], **skw))
        self.src = [mv.frame_to_device(f) for f in frames]
        self.sf = self.sup.build(self.src)
        self.analyses, self.host = {}, {}

    def analyse(self, isb, delta, akw):
        key = (isb, delta, tuple(sorted(akw.items())))
        if key not in self.analyses:
            self.analyses[key] = self.mv.Analyse(self.sup, isb=isb, delta=delta, **akw)
        return self.analyses[key]

    def sup_np(self, n):
        if n not in self.host:
            self.host[n] = [self.mv.plane_to_numpy(self.sf[n][p], self.sup.info.plane_width[p], self.sup.dtype) for p in range(self.sup.nplanes)]
        return self.host[n]

    def pitch(self):
        return [p.stride(0) for p in self.src[0]]


def _pipe(mv, geo, n, frames=None, tag=None, noise=3):
    fmt, w, h, bits, skw, _ = geo
    key = (fmt, w, h, bits, tuple(sorted(skw.items())), n, tag, noise)
    if key not in _pipes:
        _pipes[key] = Pipe(mv, frames if frames is not None else dc.clip(w, h, bits, n, fmt, noise=noise), w, h, bits, fmt, skw)
    return key, _pipes[key]


def _job(mv, geo, n, target, radius, **kw):
    """-> (pipe, analysis data, frame numbers of the 2 * radius references or None, their searched blobs on the device); searched once per
    (clip, target) at the largest radius asked for so far"""
    key, pipe = _pipe(mv, geo, n, **kw)
    akw = geo[5]
    have = _jobs.get((key, target))
    if have is None or len(have[1]) < 2 * radius:
        nrefs, blobs = [], []
        for r, isb, d, nref in dc.neighbours(target, radius, n):
            an = pipe.analyse(isb, d, akw)
            blobs.append(an.run([(pipe.sf[target], pipe.sf[nref] if nref is not None else None)])[0])
            nrefs.append(nref)
        have = _jobs[(key, target)] = (nrefs, blobs, an.ad)
    return pipe, have[2], have[0][:2 * radius], have[1][:2 * radius]


def _gpu_job(pipe, target, nrefs, blobs):
    return (pipe.src[target], [pipe.sf[n] if n is not None else None for n in nrefs], blobs)


def _planes(mv, pipe, out):
    import torch
    torch.cuda.synchronize()
    return [mv.plane_to_numpy(out[p], pipe.frames[0][p].shape[1], pipe.frames[0][p].dtype) for p in range(len(pipe.frames[0]))]


def _same(got, want, what):
    assert len(got) == len(want)
    for p in range(len(want)):
        assert pl.first_diff(got[p], want[p]) == "", "%s plane %d" % (what, p)


def _restated(oracle, mv, pipe, ad, radius, dkw, target, nrefs, blobs, info):
    """the restatement's output for one job, and the restatement (for its plan)"""
    ref = dc.restatement(oracle, radius, ad, info["thsad_d"], info["thsadc_d"], dkw, gray=pipe.fmt == "gray")
    want = ref.frame(pipe.frames[target], [pipe.sup_np(n) if n is not None else None for n in nrefs], [np.asarray(b.cpu().numpy()) for b in blobs])
    return want, ref


# ------------------------------------------------------------------------------------------------ radius 1..6: the new kernels against the old

SMALL = [dc.A, dc.B, ("420", 160, 96, 8, dict(pel=1), dict(blksize=8, overlap=0))]


@pytest.mark.parametrize("radius", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("geo", SMALL, ids=lambda g: "%dx%d-%dbit" % (g[1], g[2], g[3]))
def test_up_to_radius_6_the_bytes_are_degrains(mv, geo, radius):
    """the middle frame and frame 0, whose forward references lie outside the clip, in one call"""
    jobs = []
    for target in (6, 0):
        pipe, ad, nrefs, blobs = _job(mv, geo, 13, target, 6)
        jobs.append(_gpu_job(pipe, target, nrefs[:2 * radius], blobs[:2 * radius]))
    want = mv.Degrain(radius, pipe.sup, ad, pipe.pitch()).run(jobs)
    got = mv.DegrainN(radius, pipe.sup, ad, pipe.pitch()).run(jobs)
    for j, target in enumerate((6, 0)):
        w = _planes(mv, pipe, want[j])
        _same(_planes(mv, pipe, got[j]), w, "frame %d" % target)
        assert not np.array_equal(w[0], pipe.frames[target][0])


# ------------------------------------------------------------------------------------------------ beyond 6: against the restatement

@pytest.mark.parametrize("case", dc.LARGE_CASES, ids=dc.case_id)
def test_beyond_radius_6_the_bytes_are_the_restatements(oracle, mv, case):
    geo, radius, dkw = case[:6], case[6], case[7]
    n = 2 * radius + 1
    pipe, ad, nrefs, blobs = _job(mv, geo, n, radius, radius)
    dg = mv.DegrainN(radius, pipe.sup, ad, pipe.pitch(), **dkw)
    got = _planes(mv, pipe, dg.run([_gpu_job(pipe, radius, nrefs, blobs)])[0])
    want, ref = _restated(oracle, mv, pipe, ad, radius, dkw, radius, nrefs, blobs, dg.info())
    ok, what = dc.far_shares_ok(ref)
    assert ok, what
    _same(got, want, dc.case_id(case))


@pytest.mark.parametrize("gen", dc.RANGE_GENS)
def test_sample_range_at_radius_8(oracle, mv, gen):
    pipe, ad, nrefs, blobs = _job(mv, dc.RANGE_GEO, 17, 8, 8, frames=dc.range_clip(gen, 17), tag=gen)
    dg = mv.DegrainN(8, pipe.sup, ad, pipe.pitch())
    got = _planes(mv, pipe, dg.run([_gpu_job(pipe, 8, nrefs, blobs)])[0])
    want, ref = _restated(oracle, mv, pipe, ad, 8, {}, 8, nrefs, blobs, dg.info())
    ok, what = dc.far_shares_ok(ref)
    assert ok, what
    _same(got, want, gen)


def test_references_beyond_distance_4_unusable_leave_degrain4(mv):
    """radius 10; every backward reference beyond distance 4 is a frame outside the clip (NULL planes, a searched blob all the same), every forward one
    carries a blob with one block too many above thscd1 (tests/vector_fields.py scene_count)"""
    import torch
    pipe, ad, nrefs, blobs = _job(mv, dc.A, 21, 10, 10)
    refs = [pipe.sf[n] for n in nrefs]
    th, s1, s2 = vector_fields.scaled_thresholds(ad, 400)
    cut_refs, cut_blobs = list(refs), list(blobs)
    for r, isb, d, _ in dc.neighbours(10, 10, 21):
        if d > 4 and isb:
            cut_refs[r] = None
        elif d > 4:
            edited = vector_fields.scene_count(blobs[r].cpu().numpy(), ad, 300 + r, s1, s2 + 1, th)
            cut_blobs[r] = torch.from_numpy(edited).to(blobs[r].device)
    want = _planes(mv, pipe, mv.Degrain(4, pipe.sup, ad, pipe.pitch()).run([(pipe.src[10], refs[:8], blobs[:8])])[0])
    dg = mv.DegrainN(10, pipe.sup, ad, pipe.pitch())
    _same(_planes(mv, pipe, dg.run([(pipe.src[10], cut_refs, cut_blobs)])[0]), want, "truncated")
    full = _planes(mv, pipe, dg.run([(pipe.src[10], refs, blobs)])[0])
    assert not np.array_equal(full[0], want[0])  # (with them the far references do change the frame)


@pytest.mark.parametrize("target,what", [(0, "no forward references"), (16, "no backward references")])
def test_clip_ends(oracle, mv, target, what):
    pipe, ad, nrefs, blobs = _job(mv, dc.A, 17, target, 8)
    assert [n is None for n in nrefs] == [bool(r % 2) == (target == 0) for r in range(16)]
    dg = mv.DegrainN(8, pipe.sup, ad, pipe.pitch())
    got = _planes(mv, pipe, dg.run([_gpu_job(pipe, target, nrefs, blobs)])[0])
    want, ref = _restated(oracle, mv, pipe, ad, 8, {}, target, nrefs, blobs, dg.info())
    w = ref.plan[0][1]
    inside = [r for r in range(12, 16) if nrefs[r] is not None]
    assert np.mean(w[:, inside] > 0) >= dc.FAR_USED and not np.any(w[:, [r for r in range(16) if nrefs[r] is None]])
    _same(got, want, what)


def test_a_job_without_any_reference_returns_the_source(mv):
    """every reference frame outside the clip (NULL planes); the blobs are searched ones, valid, and must not be looked at"""
    pipe, ad, nrefs, blobs = _job(mv, dc.A, 17, 8, 8)
    got = _planes(mv, pipe, mv.DegrainN(8, pipe.sup, ad, pipe.pitch()).run([(pipe.src[8], [None] * 16, blobs)])[0])
    _same(got, pipe.frames[8], "no reference")
    # ... nor dereferenced: no blob at all
    got = _planes(mv, pipe, mv.DegrainN(8, pipe.sup, ad, pipe.pitch()).run([(pipe.src[8], [None] * 16, [None] * 16)])[0])
    _same(got, pipe.frames[8], "no reference, no blob")


def test_identical_frames_are_returned_unchanged_at_radius_24(mv):
    """a static clip without noise: every vector 0, every SAD 0, every weight 5 and WSrc 16 (tests/test_degrain_n_cases.py), (128 + 256 s) >> 8 = s, and
    the windows of an 8-bit frame give s back"""
    fmt, w, h, bits, skw, akw = dc.A
    frame = dc.clip(w, h, bits, 1, fmt, noise=0)[0]
    pipe, ad, nrefs, blobs = _job(mv, dc.A, 49, 24, 24, frames=[frame] * 49, tag="static")
    for b in blobs[::7]:
        _, _, sad = pl.blob_vectors(b.cpu().numpy(), ad)
        assert not sad.any()
    got = _planes(mv, pipe, mv.DegrainN(24, pipe.sup, ad, pipe.pitch()).run([_gpu_job(pipe, 24, nrefs, blobs)])[0])
    _same(got, frame, "static clip")


def test_four_jobs_in_one_call_are_the_four_run_singly(mv):
    jobs = []
    for target in (8, 9, 0, 19):
        pipe, ad, nrefs, blobs = _job(mv, dc.A, 20, target, 8)
        jobs.append(_gpu_job(pipe, target, nrefs, blobs))
    dg = mv.DegrainN(8, pipe.sup, ad, pipe.pitch(), thsad=1600, thsad2=400)
    together = [_planes(mv, pipe, o) for o in dg.run(jobs)]
    for j, job in enumerate(jobs):
        _same(together[j], _planes(mv, pipe, dg.run([job])[0]), "job %d" % j)
    assert not np.array_equal(together[0][0], together[1][0])
