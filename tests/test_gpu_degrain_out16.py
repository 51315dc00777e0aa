"""GPU: mv.DegrainN with out16 -- an 8-bit clip, 8-bit super frames and the 8-bit search's vectors, written as 16-bit planes -- through the
C ABI, byte for byte against tests/degrain_out16_ref.py: the 16-bit path of the restatement that tests/test_degrain_n_ref.py holds to the
oracle, on samples shifted left by 8 with the 8-bit filter's own threshold tables (info()) and 8-bit scene-change thresholds.
tests/test_degrain_out16_ref.py ties that yardstick to the oracle's 8-bit Degrain.

Clips, vectors and geometries are those of tests/test_gpu_degrain_n.py (its 8-bit cases, searched once for both files).  Every case beyond
radius 6 meets degrain_n_cases.far_shares_ok -- most far references carry a weight and some carry none -- which tests/test_degrain_n_cases.py
and tests/test_degrain_out16_ref.py show on the CPU and which is asserted here from the yardstick's plan."""
import numpy as np
import pytest

import degrain_n_cases as dc
import degrain_out16_ref as o16
import pipeline as pl
import sample_range as sr
from test_gpu_degrain_n import _gpu_job, _job, _same

pytestmark = pytest.mark.gpu


def _planes16(mv, pipe, out):
    import torch
    torch.cuda.synchronize()
    return [mv.plane_to_numpy(out[p], pipe.frames[0][p].shape[1], np.uint16) for p in range(len(pipe.frames[0]))]


def _planes8(mv, pipe, out):
    import torch
    torch.cuda.synchronize()
    return [mv.plane_to_numpy(out[p], pipe.frames[0][p].shape[1], np.uint8) for p in range(len(pipe.frames[0]))]


def _shifted(frame):
    return [p.astype(np.uint16) << 8 for p in frame]


def _restated(oracle, pipe, ad, radius, dkw, target, nrefs, blobs, info):
    ref = o16.restatement(oracle, radius, ad, info["thsad_d"], info["thsadc_d"], dkw, gray=pipe.fmt == "gray")
    want = o16.frame(ref, pipe.frames[target], [pipe.sup_np(n) if n is not None else None for n in nrefs], [np.asarray(b.cpu().numpy()) for b in blobs])
    return want, ref


def _run_case(oracle, mv, geo, radius, dkw, **kw):
    """the middle frame of 2 * radius + 1 against the yardstick; -> (the GPU's planes, the pipe)"""
    n = 2 * radius + 1
    pipe, ad, nrefs, blobs = _job(mv, geo, n, radius, radius, **kw)
    dg = mv.DegrainN(radius, pipe.sup, ad, pipe.pitch(), out16=True, **dkw)
    assert dg.out_bits == 16
    got = _planes16(mv, pipe, dg.run([_gpu_job(pipe, radius, nrefs, blobs)])[0])
    want, ref = _restated(oracle, pipe, ad, radius, dkw, radius, nrefs, blobs, dg.info())
    if radius > 6:
        ok, what = dc.far_shares_ok(ref)
        assert ok, what
    assert np.count_nonzero(ref.plan[0][1]) > 0
    _same(got, want, "out16")
    return got, pipe


# ------------------------------------------------------------------------------------------------ radius and geometry

@pytest.mark.parametrize("radius", [1, 3, 6])
def test_small_radii_on_cells_of_4_and_2(oracle, mv, radius):
    got, pipe = _run_case(oracle, mv, dc.A, radius, {})
    assert np.count_nonzero(got[0] & 255) > got[0].size // 4  # more than the 8-bit result shifted


# the 8-bit rows of LARGE_CASES: radius 7, 8, 9, 12 and 24 on A (8x8 overlap 4), blocks side by side, 32x32 overlap 16 (cells of 8: the 16-byte store), 8x4, 4/2
# (one-sample cells), pel 1, 4:4:4, Gray, plane 0..4, a limit (of 1 / 0 in output units), the thsad2 fall-off at radius 8 and 24; then 4:2:2, B's size
# (204 wide: an uncovered strip of 4 and a partial last cell of 8) and the limits the out16 definition names
CASES = [c for c in dc.LARGE_CASES if c[3] == 8] + [
    ("422", 160, 96, 8, {}, dc.B168, 7, {}),
    ("420", 204, 116, 8, {}, dc.B168, 8, {}),
    dc.A + (8, dict(limit=256, limitc=0)),
    dc.A + (8, dict(limit=65534)),          # active, never binding: no sample is above 65280
    dc.A + (8, dict(limit=300, plane=3)),
]


@pytest.mark.parametrize("case", CASES, ids=dc.case_id)
def test_the_bytes_are_the_yardsticks(oracle, mv, case):
    geo, radius, dkw = case[:6], case[6], case[7]
    got, pipe = _run_case(oracle, mv, geo, radius, dkw)
    src = _shifted(pipe.frames[radius])
    if dkw.get("limit") == 256:  # the limit binds somewhere and limitc = 0 returns the source
        d = np.abs(got[0].astype(np.int64) - src[0])
        assert int(d.max()) == 256 and np.count_nonzero(d == 256) > 100
        assert np.array_equal(got[1], src[1]) and np.array_equal(got[2], src[2])
    if dkw.get("limit") == 65534:
        free, _ = _run_case(oracle, mv, geo, radius, {})
        _same(got, free, "limit 65534 against no limit")
    if "plane" in dkw:
        processed = [(1, 2, 4, 6, 7)[dkw["plane"]] >> p & 1 for p in range(3)]
        for p in range(3):
            assert processed[p] != np.array_equal(got[p], src[p]), "plane %d" % p


# ------------------------------------------------------------------------------------------------ the ends of the 8-bit range

def _range_clip(gen, n):
    _, w, h, _, _, _ = dc.A
    return sr.step(w, h, 8, n, 0, 255) if gen == "step" else sr.rails(w, h, 8, n, motion=(1, 0))


@pytest.mark.parametrize("gen", ["step", "rails"])
def test_sample_range_at_radius_8(oracle, mv, gen):
    got, pipe = _run_case(oracle, mv, dc.A, 8, {}, frames=_range_clip(gen, 17), tag=gen + "8")
    if gen == "rails":
        assert np.count_nonzero(got[0] == 0) > 1000 and np.count_nonzero(got[0] == 65280) > 1000 and int(got[0].max()) == 65280


@pytest.mark.parametrize("level", [255, 0])
@pytest.mark.parametrize("akw", [dc.B84, dict(blksize=8, overlap=0)], ids=["overlap4", "overlap0"])
def test_a_flat_clip_keeps_its_level(oracle, mv, level, akw):
    """every sample 255: every block's sum is 256 * 255 and the output 65280 everywhere (not 65535: the output is the sum, not a rescaling);
    every sample 0: 0.  Radius 6 -- every weight is above 0, which the share condition of the larger radii rules out"""
    fmt, w, h, bits, skw, _ = dc.A
    geo = (fmt, w, h, bits, skw, akw)
    frame = [np.full_like(p, level) for p in dc.clip(w, h, bits, 1, fmt)[0]]
    got, pipe = _run_case(oracle, mv, geo, 6, {}, frames=[frame] * 13, tag="flat%d" % level)
    for p in range(3):
        assert np.all(got[p] == level * 256), "plane %d" % p


# ------------------------------------------------------------------------------------------------ degenerate jobs

@pytest.mark.parametrize("target,what", [(0, "no forward references"), (16, "no backward references")])
def test_clip_ends(oracle, mv, target, what):
    pipe, ad, nrefs, blobs = _job(mv, dc.A, 17, target, 8)
    assert [n is None for n in nrefs] == [bool(r % 2) == (target == 0) for r in range(16)]
    dg = mv.DegrainN(8, pipe.sup, ad, pipe.pitch(), out16=True)
    got = _planes16(mv, pipe, dg.run([_gpu_job(pipe, target, nrefs, blobs)])[0])
    want, ref = _restated(oracle, pipe, ad, 8, {}, target, nrefs, blobs, dg.info())
    w = ref.plan[0][1]
    inside = [r for r in range(12, 16) if nrefs[r] is not None]
    assert np.mean(w[:, inside] > 0) >= dc.FAR_USED and not np.any(w[:, [r for r in range(16) if nrefs[r] is None]])
    _same(got, want, what)


def test_a_job_without_any_reference_returns_the_source_shifted(mv):
    pipe, ad, nrefs, blobs = _job(mv, dc.A, 17, 8, 8)
    dg = mv.DegrainN(8, pipe.sup, ad, pipe.pitch(), out16=True, limit=1000)
    want = _shifted(pipe.frames[8])
    _same(_planes16(mv, pipe, dg.run([(pipe.src[8], [None] * 16, blobs)])[0]), want, "no reference")
    _same(_planes16(mv, pipe, dg.run([(pipe.src[8], [None] * 16, [None] * 16)])[0]), want, "no reference, no blob")


def test_four_jobs_in_one_call_are_the_four_run_singly(mv):
    jobs = []
    for target in (8, 9, 0, 19):
        pipe, ad, nrefs, blobs = _job(mv, dc.A, 20, target, 8)
        jobs.append(_gpu_job(pipe, target, nrefs, blobs))
    dg = mv.DegrainN(8, pipe.sup, ad, pipe.pitch(), out16=True, thsad=1600, thsad2=400)
    together = [_planes16(mv, pipe, o) for o in dg.run(jobs)]
    for j, job in enumerate(jobs):
        _same(together[j], _planes16(mv, pipe, dg.run([job])[0]), "job %d" % j)
    assert not np.array_equal(together[0][0], together[1][0])


# ------------------------------------------------------------------------------------------------ the reference-pinned 8-bit kernels

SIDE_BY_SIDE = [(("420", 160, 96, 8, {}, dict(blksize=8, overlap=0)), 8), (("420", 160, 96, 8, dict(pel=1), dict(blksize=8, overlap=0)), 3)]


@pytest.mark.parametrize("geo,radius", SIDE_BY_SIDE, ids=["pel2-r8", "pel1-r3"])
def test_side_by_side_rounds_to_the_8_bit_objects_bytes(mv, geo, radius):
    """blocks side by side, no limit: out16 is the sum S and the 8-bit DegrainN's byte is (S + 128) >> 8 -- the same job through both objects"""
    n = 2 * radius + 1
    pipe, ad, nrefs, blobs = _job(mv, geo, n, radius, radius)
    job = _gpu_job(pipe, radius, nrefs, blobs)
    got16 = _planes16(mv, pipe, mv.DegrainN(radius, pipe.sup, ad, pipe.pitch(), out16=True).run([job])[0])
    got8 = _planes8(mv, pipe, mv.DegrainN(radius, pipe.sup, ad, pipe.pitch()).run([job])[0])
    assert not np.array_equal(got8[0], pipe.frames[radius][0])
    for p in range(3):
        assert pl.first_diff(((got16[p].astype(np.int64) + 128) >> 8).astype(np.uint8), got8[p]) == "", "plane %d" % p


# ------------------------------------------------------------------------------------------------ nothing outside the destination's samples is written

@pytest.mark.parametrize("geo", [dc.A, ("420", 204, 116, 8, {}, dc.B168)], ids=["128x96", "204x116"])
def test_guard_band_around_the_destination_is_untouched(oracle, mv, geo):
    """each 16-bit plane sits inside an allocation filled with 0xA5: 8 rows above it, 8 rows below it (the rows past the plane's last row,
    which a row index that ran on by a pitch would reach), and the bytes of every row beyond 2 * width up to a pitch that is 256 bytes
    longer than the default"""
    import torch
    radius, G = 8, 8
    pipe, ad, nrefs, blobs = _job(mv, geo, 2 * radius + 1, radius, radius)
    pitch = [(2 * f.shape[1] + 255) // 256 * 256 + 256 for f in pipe.frames[0]]
    dg = mv.DegrainN(radius, pipe.sup, ad, pipe.pitch(), dst_pitch=pitch, out16=True)
    assert dg.dst_pitch == pitch
    big = [torch.full((p.shape[0] + 2 * G, dg.dst_pitch[i]), 0xA5, dtype=torch.uint8, device=p.device) for i, p in enumerate(pipe.src[radius])]
    out = [b[G:b.shape[0] - G] for b in big]
    dg.run([_gpu_job(pipe, radius, nrefs, blobs)], out=[out])
    got = _planes16(mv, pipe, out)
    want, _ = _restated(oracle, pipe, ad, radius, {}, radius, nrefs, blobs, dg.info())
    _same(got, want, "inside the guard band")
    for p, b in enumerate(big):
        host = b.cpu().numpy()
        rowbytes = 2 * pipe.frames[0][p].shape[1]
        assert rowbytes < host.shape[1]
        assert np.all(host[:G] == 0xA5) and np.all(host[-G:] == 0xA5), "plane %d: rows outside the plane were written" % p
        assert np.all(host[G:-G, rowbytes:] == 0xA5), "plane %d: bytes beyond the row's samples were written" % p
