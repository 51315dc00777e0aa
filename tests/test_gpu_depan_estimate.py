"""GPU tests of mv.DepanEstimate (csrc/mvx_depan_fft.hip) through the Python package.  A single-precision FFT cannot equal FFTW's bit for bit, so
the three checks of tests/depan_estimate_checks.py replace byte parity: the spectrum against a double-precision FFT within the bound of a
single-precision radix FFT; every discrete result equal to the restatement tests/depan_estimate_ref.py with the double FFT; dx, dy, zoom and trust
within 4 D of it, D being the distance between the restatements with two independent FFTs, computed here.

The windows are those of tests/depan_estimate_cases.py: 8 x 8, 32 x 16, 16 x 64, 256 x 128, 8192 x 8, 8 x 8192 and, on either axis, 256, 512, 1024,
2048, 4096 and 8192 -- each on one side of a change of the transforms per workgroup (32, 16, 8, 4, 2, 1); a workgroup's LDS stays within 64 KiB, so
capacity adds no path.  Each at 8 and 16 bits, one at 10; windows with an odd origin; every plane with a pitch that is no multiple of its window.
Each case runs on the GPU once; the tests share the results."""
import numpy as np
import pytest

import depan_estimate_cases as dc
import depan_estimate_checks as ck

pytestmark = pytest.mark.gpu
f32 = np.float32
_runs = {}


def _dev(plane):
    """a device plane whose pitch is its row plus 6 samples: no multiple of any window"""
    import torch
    h, rowbytes = plane.shape[0], plane.shape[1] * plane.itemsize
    t = torch.full((h, rowbytes + 6 * plane.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    t[:, :rowbytes] = torch.from_numpy(plane.view(np.uint8).reshape(h, rowbytes)).to("cuda")
    return t


def _filter(mv, c):
    return mv.DepanEstimate(c.width, c.height, c.bits, **c.kw)


def _run(mv, c):
    if c.name not in _runs:
        g = _filter(mv, c)
        prev, cur = c.frames()
        sp = g.spectra([_dev(prev), _dev(cur)])
        res, scans = g.correlate([sp[0]], [sp[1]], None if c.prop is None else [c.prop], [c.n], scans=True)
        _runs[c.name] = dict(spectra=[s.cpu().numpy() for s in sp], result=res[0], scans=scans)
    return _runs[c.name]


@pytest.mark.parametrize("c", dc.CASES, ids=repr)
def test_spectrum_within_the_bound_of_a_single_precision_fft(mv, c):
    r = _run(mv, c)
    for frame, spec in zip(c.frames(), r["spectra"]):
        assert spec.shape == (c.ref().windows, c.ref().winy, c.ref().winx // 2 + 1, 2)
        ck.assert_spectrum(c, frame, spec)


@pytest.mark.parametrize("c", dc.CASES, ids=repr)
def test_discrete_results_equal_the_double_restatement(mv, c):
    r = _run(mv, c)
    ck.assert_discrete(c, r["scans"], r["result"])


@pytest.mark.parametrize("c", dc.CASES, ids=repr)
def test_dx_dy_zoom_trust_within_four_times_the_distance_of_two_ffts(mv, c):
    ck.assert_close(c, _run(mv, c)["result"])


def test_scan_results_feed_the_host_tail_to_the_same_result(mv):
    for c in dc.CASES:
        r = _run(mv, c)
        assert _filter(mv, c).host_tail(r["scans"], None if c.prop is None else [c.prop], [c.n])[0] == r["result"]


def test_stage3_zeroing_equals_the_double_restatement(mv):
    """a clip a, a + pan, b, b: frame 2 is a scene change.  Stage 3 of the library on the library's stage-2 results gives the zeros and non-zeros
    that the restatement's stage 3 gives on the restatement's own stage-2 results with the double FFT, and values within 4 D of them"""
    a, b = dc.BY_NAME["w256x128_8bit"], dc.BY_NAME["scene_change_256x128"]
    frames = [np.ascontiguousarray(f) for f in (a.frames()[0][:128, :256], a.frames()[1][:128, :256], b.frames()[1], b.frames()[1])]
    e = dc.er.Estimate(256, 128, winx=256, winy=128, num_frames=4)
    ref = [e.pair(frames[max(0, n - 1)], frames[n], n, dc.er.FFT64) for n in range(4)]
    want = [e.finish(n, [ref[max(0, n - 1)], ref[n], ref[min(n + 1, 3)]]) for n in range(4)]
    assert [w[0] != 0 for w in want] == [False, True, False, True]
    g = mv.DepanEstimate(256, 128, winx=256, winy=128, num_frames=4)
    sp = g.spectra([_dev(f) for f in frames])
    got = g.finish(g.correlate([sp[max(0, k - 1)] for k in range(4)], sp, None, list(range(4))))
    D = ck.D()
    for m, w in zip(got, want):
        assert [v == 0 for v in m[:2]] == [v == 0 for v in w[:2]] and (m[2] == 1) == (w[2] == 1) and m[3] == 0
        assert abs(m[0] - float(w[0])) <= 4 * D["dx"] and abs(m[1] - float(w[1])) <= 4 * D["dy"] and abs(m[2] - float(w[2])) <= 4 * D["zoom"]


def test_the_same_batch_twice_and_batches_of_one_and_five_are_bit_identical(mv):
    names = ["w256x128_8bit", "w8x8192_16bit", "w8192x8_8bit", "w32x16_odd_origin", "zoom_good"]
    for c in [dc.BY_NAME[n] for n in names]:
        g = _filter(mv, c)
        prev, cur = (_dev(p) for p in c.frames())
        batches = []
        for planes in ([prev, cur] * 3, [prev, cur] * 3, [prev, cur]):
            sp = g.spectra(planes)
            idx = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)] if len(planes) == 6 else [(0, 1)]
            res, scans = g.correlate([sp[i] for i, _ in idx], [sp[j] for _, j in idx], None if c.prop is None else [c.prop] * len(idx), [c.n] * len(idx), scans=True)
            batches.append(([s.cpu().numpy().tobytes() for s in sp], [tuple(f32(r[q]).tobytes() for q in ck.QUANTITIES) for r in res],
                            [tuple(f32(v).tobytes() if isinstance(v, float) else v for v in s.values()) for s in scans]))
        assert batches[0] == batches[1]
        one = batches[2]
        assert one[0] == batches[0][0][:2] and one[1][0] == batches[0][1][0] and one[2] == batches[0][2][:len(one[2])]
        assert batches[0][1][0] == batches[0][1][2] == batches[0][1][4]     # the same pair at three places of the batch
        single = _run(mv, c)["result"]
        assert one[1][0] == tuple(f32(single[q]).tobytes() for q in ck.QUANTITIES)


def test_fields_and_pixaspect(mv):
    top, bottom = _run(mv, dc.BY_NAME["fields_prop_top"])["result"], _run(mv, dc.BY_NAME["fields_prop_bottom"])["result"]
    # (yadd + 0.5) * 2 against (yadd - 0.5) * 2: two whole lines apart, as in the double restatement, each of the two within 4 D of it
    step = lambda x, y: float(dc.BY_NAME[x].result(64)["dy"]) - float(dc.BY_NAME[y].result(64)["dy"])
    tol = 8 * ck.D()["dy"]
    assert top["dx"] == bottom["dx"] and abs(top["dy"] - bottom["dy"] - step("fields_prop_top", "fields_prop_bottom")) <= tol
    assert abs(step("fields_prop_top", "fields_prop_bottom") - 2.0) <= tol
    t1, t0 = _run(mv, dc.BY_NAME["fields_tff1_n3"])["result"], _run(mv, dc.BY_NAME["fields_tff0_n3"])["result"]
    assert abs(t0["dy"] - t1["dy"] - step("fields_tff0_n3", "fields_tff1_n3")) <= tol and step("fields_tff0_n3", "fields_tff1_n3") > 1.9   # tff = 1 at odd n is a bottom field
    g = mv.DepanEstimate(80, 40, winx=64, winy=32, fields=True)
    sp = g.spectra([_dev(p) for p in dc.BY_NAME["fields_prop_top"].frames()])
    with pytest.raises(mv.MvtoolsError) as e:
        g.correlate([sp[0]], [sp[1]], None, [1])
    assert str(e.value) == "DepanEstimate: _Field property not found in input frame. Therefore, you must pass tff argument."
    c = dc.BY_NAME["pixaspect"]
    assert abs(_run(mv, c)["result"]["dy"] - c.pan[1] / 1.0940) <= 0.5


def test_end_to_end_into_depan_compensate(mv):
    """64 x 48 frames with a planted pan: run() -> DepanCompensate with nearest interpolation, the motions unchanged"""
    import torch
    import depan_ref as dr
    c = dc.BY_NAME["auto_64x48"]
    prev, cur = c.frames()
    frames = [prev, cur, prev]
    dev = [mv.plane_to_device(f) for f in frames]
    est = mv.DepanEstimate(64, 48, num_frames=3)
    motions = est.run(dev)
    assert motions[0] == (0, 0, 1, 0)
    assert abs(motions[1][0] - c.pan[0]) <= 0.5 and abs(motions[1][1] - c.pan[1]) <= 0.5 and motions[1][2:] == (1, 0)
    assert abs(motions[2][0] + c.pan[0]) <= 0.5 and abs(motions[2][1] + c.pan[1]) <= 0.5
    comp = mv.DepanCompensate(64, 48, gray=True, subsampling=(0, 0), src_pitch=[dev[0].stride(0)], offset=1.0, subpixel=0, num_frames=3)
    src, trs, want = [], [], []
    for n in range(3):
        m = comp.map(n)
        if m is None:
            continue
        t, _ = comp.transform([motions[k] for k in range(m[1] + 1, m[2] + 1)])
        src.append([dev[m[0]]])
        trs.append(t)
        want.append(dr.compensate_frame([frames[m[0]]], t, 0, 8, (0, 0), True, 0, 0, "strict")[0])
    assert len(src) == 2
    out = comp.run(src, trs)
    torch.cuda.synchronize()
    for o, w in zip(out, want):
        assert np.array_equal(mv.plane_to_numpy(o[0], 64, np.uint8), w)
    # frame 0 warped by the motion of frame 1 lands on frame 1 wherever the source exists
    got = mv.plane_to_numpy(out[0][0], 64, np.uint8)
    inner = (slice(8, 40), slice(8, 56))
    assert np.array_equal(got[inner], cur[inner]) and not np.array_equal(prev[inner], cur[inner])


def test_zero_frames_is_a_no_op(mv):
    g = mv.DepanEstimate(64, 48)
    assert g.spectra([]) == [] and g.correlate([], []) == [] and g.run([]) == []
    lib = mv.lib()
    assert lib.mvx_depan_estimate_spectra(g.h, 0, None, 0, None, None) == 0
    assert lib.mvx_depan_estimate_correlate(g.h, 0, None, None, None, None, None, None, None) == 0
