"""GPU: every filter handle over a script of unlike calls (tests/handle_sequences.py), bit for bit against the oracle after every call.

One handle serves a whole clip in production: thousands of calls with batches of changing size, across scene changes and clip ends, from
several streams.  The scripts make one handle do that in nine calls and more, and run three times: with the library's scratch as the
allocator leaves it, and with every fresh allocation of handle-owned scratch filled with 0xA5 and with 0x5A (mvx_debug_option
"scratch_poison"; the two fills of tests/layouts.py: a value that is right by coincidence under one is wrong under the other).  The option
changes no result -- that is what these tests assert.  tests/test_handle_sequences.py holds, on the CPU, that the jobs of a script differ."""
import numpy as np
import pytest

import handle_sequences as hs
import pipeline as pl
from test_gpu_parity import dbg  # noqa: F401  (the fixture that puts a debug option back)

pytestmark = pytest.mark.gpu

POISONS = (0, 0xA5, 0x5A)


@pytest.mark.parametrize("poison", POISONS, ids=lambda v: "poison%02X" % v)
@pytest.mark.parametrize("adapter", hs.ADAPTERS, ids=lambda a: a.name)
def test_one_handle_over_unlike_calls(mv, dbg, adapter, poison):  # noqa: F811
    dbg("scratch_poison", poison)
    hs.run_script(mv, adapter)


@pytest.mark.parametrize("poison", POISONS, ids=lambda v: "poison%02X" % v)
@pytest.mark.parametrize("shape,pel", [(hs.A8, 2), (hs.B16, 4), (hs.C8, 4)], ids=["8bit-pel2", "16bit-pel4", "8bit-odd-pel4"])
def test_one_super_handle_over_builds_of_1_9_and_2_frames(oracle, mv, dbg, shape, pel, poison):  # noqa: F811
    """mvx_super_frames keeps a table of frame pointers per thread: one frame, nine, then two into super frames that earlier builds filled
    (with other pictures), and mv.Finest of the last build -- every defined sample against the oracle"""
    import torch
    dbg("scratch_poison", poison)
    w = hs.world(shape)
    osup, gsup = oracle.Super(w.w, w.h, w.bits, pel=pel), mv.Super(w.w, w.h, w.bits, pel=pel)
    src = [mv.frame_to_device(f) for f in w.frames]
    want = {}

    def check(frames, built, what):
        torch.cuda.synchronize()
        for n, sf in zip(frames, built):
            if n not in want:
                want[n] = osup.frame(w.frames[n])
            got = [mv.plane_to_numpy(sf[p], gsup.info.plane_width[p], gsup.dtype) for p in range(gsup.nplanes)]
            bad = pl.defined_equal(osup, want[n], got)
            assert not bad, "%s, frame %d differs in defined regions (plane, level, pelplane, count, y, x, oracle, gpu): %s" % (what, n, bad[:4])

    one = gsup.build(src[:1])
    check([0], one, "build of 1")
    nine = gsup.build(src[1:])
    check(range(1, 10), nine, "build of 9")
    check([0], one, "the first build after the second")
    two = gsup.build([src[hs.CUT], src[7]], out=[nine[0], one[0]])
    check([hs.CUT, 7], two, "build of 2 into used super frames")
    check(range(2, 10), nine[1:], "the rest of the build of 9 after the build of 2")
    fin = gsup.finest(two)
    torch.cuda.synchronize()
    for n, f in zip((hs.CUT, 7), fin):
        for p, wp in enumerate(osup.finest(want[n])):
            assert np.array_equal(mv.plane_to_numpy(f[p], wp.shape[1], wp.dtype), wp), "Finest of frame %d, plane %d" % (n, p)


@pytest.mark.parametrize("poison", POISONS, ids=lambda v: "poison%02X" % v)
@pytest.mark.parametrize("shape,pel", [(hs.A8, 2), (hs.C8, 4)], ids=["pel2", "odd-pel4"])
def test_one_float_super_handle_over_builds_of_1_9_and_2_frames(mv, dbg, shape, pel, poison):  # noqa: F811
    """the same on a float clip (mvx_super_create_float), every defined sample against tests/super_float_ref.py.  There is no float Finest:
    mvx_finest_frames refuses a float super clip before any launch, which the sequence ends on"""
    import super_float_ref
    import torch
    dbg("scratch_poison", poison)
    w = hs.world(shape)
    frames = w.floats()[0]
    gsup = mv.Super(w.w, w.h, 32, sample_float=True, pel=pel)
    kw = dict(sub=(1, 1), gray=False, hpad=gsup.info.hpad, vpad=gsup.info.vpad, pel=gsup.info.pel, sharp=gsup.info.sharp)
    src = [mv.frame_to_device(f) for f in frames]
    want = {}

    def check(ns, built, what):
        torch.cuda.synchronize()
        for n, sf in zip(ns, built):
            if n not in want:
                want[n] = super_float_ref.frame(frames[n], **kw)
            for p, (wp, mask) in enumerate(zip(*want[n])):
                got = mv.plane_to_numpy(sf[p], gsup.info.plane_width[p], np.float32)
                assert got.shape == wp.shape and np.array_equal(got[mask], wp[mask]), "%s, frame %d plane %d" % (what, n, p)

    one = gsup.build(src[:1])
    check([0], one, "build of 1")
    nine = gsup.build(src[1:])
    check(range(1, 10), nine, "build of 9")
    check([0], one, "the first build after the second")
    two = gsup.build([src[hs.CUT], src[7]], out=[nine[0], one[0]])
    check([hs.CUT, 7], two, "build of 2 into used super frames")
    check(range(2, 10), nine[1:], "the rest of the build of 9 after the build of 2")
    with pytest.raises(mv.MvtoolsError, match="float super clips are not supported"):
        gsup.finest(two)
    check([hs.CUT, 7], two, "the build of 2 after the refused Finest")


def _estimate_cases(tag):
    """five pairs of frames of one geometry: four pans on four canvases and a scene change"""
    import depan_estimate_cases as ec
    geo = {"256x128": ((256, 128, 8), dict(winx=256, winy=128), {}, [(5, -3), (-7, 2), (1, 1), (-2, -4)]),
           "fields-64x32": ((80, 40, 8), dict(winx=64, winy=32, fields=True, trust=20.0), dict(n=2), [(-3, -2), (4, 2), (7, -3), (-5, 1)]),
           "odd-origin-16bit": ((91, 29, 16), dict(winx=64, winy=16, wleft=21, wtop=5, trust=20.0), {}, [(-9, 1), (3, 2), (6, -1), (-2, -3)])}[tag]
    (w, h, bits), kw, extra, pans = geo
    cases = [ec.Case("seq-%s-%d" % (tag, k), w, h, bits, "pan", 600 + k, pan=pan, prop=(k & 1) if kw.get("fields") else None, **dict(kw, **extra)) for k, pan in enumerate(pans)]
    cases.insert(2, ec.Case("seq-%s-cut" % tag, w, h, bits, "scene_change", 650, prop=1 if kw.get("fields") else None, **dict(kw, **extra)))
    return cases


@pytest.mark.parametrize("poison", POISONS, ids=lambda v: "poison%02X" % v)
@pytest.mark.parametrize("tag", ["256x128", "fields-64x32", "odd-origin-16bit"])
def test_one_depan_estimate_handle_over_batches_of_5_1_and_5(mv, dbg, tag, poison):  # noqa: F811
    """mvx_depan_estimate keeps spectra, correlation surfaces and peak records per batch: five pairs, then the scene change alone in the first
    pair's place, then the five in another order -- every result within the bounds of tests/test_gpu_depan_estimate.py (the discrete results
    equal to the double restatement's, dx, dy, zoom and trust within four times the distance of two FFTs)"""
    import depan_estimate_checks as ck
    from test_gpu_depan_estimate import _dev
    dbg("scratch_poison", poison)
    cases = _estimate_cases(tag)
    assert cases[2].result(64)["dx"] == 0 and all(c.result(64)["dx"] != 0 for c in cases[:2] + cases[3:]), "the cut is a scene change, the pans are not"
    g = mv.DepanEstimate(cases[0].width, cases[0].height, cases[0].bits, **cases[0].kw)
    windows = cases[0].ref().windows
    dev = [[_dev(p) for p in c.frames()] for c in cases]
    for order in ((0, 1, 2, 3, 4), (2,), (4, 3, 0, 2, 1), (1,), (3, 2)):
        sp = g.spectra([pl_ for k in order for pl_ in dev[k]])
        props = None if cases[0].prop is None else [cases[k].prop for k in order]
        res, scans = g.correlate(sp[0::2], sp[1::2], props, [cases[k].n for k in order], scans=True)
        assert len(res) == len(order) and len(scans) == len(order) * windows
        for i, k in enumerate(order):
            ck.assert_discrete(cases[k], scans[i * windows:(i + 1) * windows], res[i])
            ck.assert_close(cases[k], res[i])


def test_scratch_poison_takes_a_byte_or_zero(mv, dbg):  # noqa: F811
    dbg("scratch_poison", 0)
    for bad in (-1, 256):
        with pytest.raises(mv.MvtoolsError):
            mv.debug_option("scratch_poison", bad)
