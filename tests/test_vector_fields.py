"""CPU checks that the crafted vector fields of tests/vector_fields.py are what their recipes claim, for every case that
tests/test_gpu_vector_fields.py runs (the lists are shared): a GPU case may only be listed if its field passes here.  The fields are built
exactly as the GPU file builds them (vector_fields.case_editor, the same blob indices) on the oracle's default blob with the validity word
set: every recipe overwrites what it depends on, so no search is needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_ref
import vector_fields as vf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = {"420": dict(subsampling=(1, 1)), "444": dict(subsampling=(0, 0)), "422": dict(subsampling=(1, 0)), "gray": dict(gray=True)}


def _blank(oracle, sup, **akw):
    """(analysis data, a structurally complete blob with validity 1) of an Analyse with these arguments"""
    an = oracle.Analyse(sup, **akw)
    blob = an.frame(sup.alloc(), None)
    blob[4:8].view(np.int32)[0] = 1
    return an.ad, blob


def _usable(oracle, ad, blob, thscd1, thscd2):
    a = oracle.AnalysisData.from_buffer_copy(bytes(ad))
    b = np.ascontiguousarray(blob)
    return oracle.lib().mvo_blob_is_usable(C.byref(a), C.c_void_p(b.ctypes.data), thscd1, thscd2)


def _fields(oracle, consumer, case):
    """[(edited blob, analysis data, blob index)] of one case, in the order and with the indices of the GPU file, and a context dict"""
    recipe = case[-1]
    ctx = {}
    if consumer == "degrain":
        w, h, bits, radius, skw, akw, kw = case[:7]
        sup = oracle.Super(w, h, bits, **skw)
        jobs = [dict(isb=isb, delta=d, **akw) for d in range(1, radius + 1) for isb in (1, 0)]
    elif consumer == "compensate":
        w, h, bits, skw, akw, kw, shift = case[:7]
        sup = oracle.Super(w, h, bits, **skw)
        jobs = [dict(akw, isb=1, **(dict(fields=1) if shift is not None else {}))]
    elif consumer == "blockfps":
        w, h, bits, akw, kw = case[:5]
        sup = oracle.Super(w, h, bits)
        akw = dict(akw)
        nf = 3 + akw.get("delta", 1)
        jobs = [dict(akw, isb=isb, num_frames=nf) for isb in (1, 0) for _ in range(nf)]
        ctx["nf"] = nf
    elif consumer == "recalculate":
        bits, pel_old, pel_new, akw, kw = case[:5]
        sup = oracle.Super(192, 128, bits, pel=pel_old)
        jobs = [dict(akw, isb=1, num_frames=2)] * 2
    else:
        fmt, w, h, bits, skw, akw, kw = case[:7]
        sup = oracle.Super(w, h, bits, **dict(FORMATS[fmt], **skw))
        akw = dict(akw)
        both = consumer != "flow"
        jobs = [dict(akw, isb=isb, num_frames=4) for isb in ((1, 0) if both else (akw.pop("isb"),)) for _ in range(4)]
        ctx["nf"] = 4
    ctx["sup"], ctx["kw"] = sup, kw
    blanks = [_blank(oracle, sup, **j) for j in jobs]
    rc = oracle.Recalculate(oracle.Super(192, 128, case[0], pel=case[2]), blanks[0][0], **kw) if consumer == "recalculate" else None
    ctx["rc"] = rc
    edit = vf.case_editor(consumer, recipe, kw, rc)
    return [(edit(blob, ad, i), ad, i) for i, (ad, blob) in enumerate(blanks)], ctx


ALL = [(name, case) for name, cases in (("degrain", vf.DEGRAIN_CASES + [vf.FULL_DEGRAIN]), ("compensate", vf.COMPENSATE_CASES), ("blockfps", vf.BLOCKFPS_CASES),
                                        ("recalculate", vf.RECALC_CASES), ("flowinter", vf.FLOWINTER_CASES + [vf.FULL_FLOWFPS]), ("flow", vf.FLOW_CASES),
                                        ("flowblur", vf.BLUR_CASES)) for case in cases]
of = lambda name: [pytest.param(c, k, id="%s-%d-%s" % (c, i, k[-1])) for i, (c, k) in enumerate(ALL) if k[-1].name == name]


def test_every_recipe_is_listed_and_seeds_are_distinct():
    assert {k[-1].name for _, k in ALL} == {"limits", "sad_edges", "scene_count", "occlusion", "invalid"}
    seeds = sorted(k[-1].seed for _, k in ALL)
    assert all(b - a >= 10 for a, b in zip(seeds, seeds[1:])), "two cases would share the seed of a blob"


def test_level_walk_matches_the_oracles(oracle):
    """vector_fields.level_span walks the size headers as Fakery.c:110-121 does; on a divided clip (an extra array after level 0) too"""
    sup = oracle.Super(192, 128, 8)
    frames = [sup.frame([np.full((128, 192), 60 + 9 * k, np.uint8), np.full((64, 96), 128, np.uint8), np.full((64, 96), 128, np.uint8)]) for k in range(2)]
    for akw in (dict(blksize=16, overlap=8), dict(blksize=16, overlap=8, divide=2), dict(blksize=8, overlap=0, levels=1)):
        an = oracle.Analyse(sup, isb=1, **akw)
        blob = an.frame(frames[0], frames[1])
        ad = oracle.AnalysisData.from_buffer_copy(bytes(an.ad))
        oracle.lib().mvo_blob_level0.restype = C.c_void_p
        want = oracle.lib().mvo_blob_level0(C.byref(ad), C.c_void_p(blob.ctypes.data)) - blob.ctypes.data
        off, by, bx = vf.level_span(blob, ad)
        assert (off, by, bx) == (want, ad.nBlkY, ad.nBlkX), akw


@pytest.mark.parametrize("consumer,case", of("limits"))
def test_limits_fields(oracle, consumer, case):
    fields, ctx = _fields(oracle, consumer, case)
    margin = case[-1].kw.get("margin", 0)
    phases, parity = set(), set()
    for blob, ad, i in fields:
        xy, sad = vf.records(blob, ad)
        vx, vy = xy[:, :, 0].astype(np.int64), xy[:, :, 1].astype(np.int64)
        pel, lp = ad.nPel, {1: 0, 2: 1, 4: 2}[ad.nPel]
        X = (np.arange(ad.nBlkX, dtype=np.int64) * (ad.nBlkSizeX - ad.nOverlapX))[None, :]
        Y = (np.arange(ad.nBlkY, dtype=np.int64) * (ad.nBlkSizeY - ad.nOverlapY))[:, None]
        # the block rectangle, in sub-pel units from the padded plane's first sample, lies inside the padded plane -- also after the
        # +-margin that a field shift may add
        x0, y0 = (X + ad.nHPadding) * pel + vx, (Y + ad.nVPadding) * pel + vy
        assert (x0 - margin).min() >= 0 and (x0 + margin + ad.nBlkSizeX * pel).max() <= (ad.nWidth + 2 * ad.nHPadding) * pel, i
        assert (y0 - margin).min() >= 0 and (y0 + margin + ad.nBlkSizeY * pel).max() <= (ad.nHeight + 2 * ad.nVPadding) * pel, i
        xmin, xmax, ymin, ymax = vf.legal_rect(ad, margin)
        for hit in (vx == xmin[None, :], vx == xmax[None, :], vy == ymin[:, None], vy == ymax[:, None]):
            assert hit.any(), "a limit that no block sits on (blob %d)" % i
        assert max(np.abs(vx).max(), np.abs(vy).max()) <= 32767
        assert sad.min() >= 0 and sad.max() <= (64 if case[-1].kw.get("sad") is None else vf.scaled_thresholds(ad, 400)[1])
        _sad_masks_saturate_and_not(consumer, ctx, sad, ad)
        phases |= set(zip((vx % pel).ravel().tolist(), (vy % pel).ravel().tolist()))
        parity |= set((((X * pel + vx) >> lp) & 1).ravel().tolist())
    assert len(phases) == pel * pel, "sub-pel phase pairs missing: %s" % sorted(phases)
    assert parity == {0, 1}, "one parity of the luma start sample only (the Degrain shadow plane)"
    if consumer in ("flowinter", "flow", "flowblur"):
        _upsizer_clamps_both_ways(fields, ctx, consumer)


def _sad_masks_saturate_and_not(consumer, ctx, sad, ad):
    """BlockFPS modes 6-8 read SAD masks instead of occlusion masks: their fields must hold SADs on both sides of the cut at 255"""
    if consumer == "blockfps" and ctx["kw"].get("mode", 3) >= 6:
        l = vf.sad_mask_values(sad, ad, float(ctx["kw"].get("ml", 100.0)))
        assert (l > 255).any() and ((l >= 1) & (l < 255)).any() and _usable_default(ad, sad)


def _usable_default(ad, sad):
    return np.count_nonzero(sad > vf.scaled_thresholds(ad, 400)[1]) == 0


def _upsizer_clamps_both_ways(fields, ctx, consumer):
    """the int16 upsizer of the flow filters (SimpleResize.cpp:99-119) limits at its lower and at its upper limit on these fields"""
    low = high = 0
    for blob, ad, i in fields[:2] + fields[-2:]:
        xy, _ = vf.records(blob, ad)
        f = flow_ref.Flow(ad, ad, 4, 1, ad.nHPadding, ad.nVPadding) if consumer != "flowblur" else None
        XP, YP = (f.XP, f.YP) if f else (ad.nBlkX, ad.nBlkY)
        dw, dh = (f.wP, f.hP) if f else (ad.nWidth, ad.nHeight)
        S = flow_ref.small_fields(xy[:, :, 0], xy[:, :, 1], XP, YP) if f else (xy[:, :, 0].astype(np.int16), xy[:, :, 1].astype(np.int16))
        for comp, horizontal in ((0, True), (1, False)):
            res, lo, hi = flow_ref.upsize_i16_parts(S[comp], dw, dh, ad.nWidth, ad.nHeight, ad.nPel, horizontal)
            low += int(np.count_nonzero(res < lo))
            high += int(np.count_nonzero(res > hi))
    assert low > 0 and high > 0, (low, high)


@pytest.mark.parametrize("consumer,case", of("sad_edges"))
def test_sad_edges_fields(oracle, consumer, case):
    fields, ctx = _fields(oracle, consumer, case)
    kw, recipe = ctx["kw"], case[-1]
    weights = []
    for blob, ad, i in fields:
        _, sad = vf.records(blob, ad)
        if consumer == "recalculate":
            th = vf.recalculate_threshold(ctx["rc"])
        else:
            thsad = kw.get("thsad", 400 if consumer == "degrain" else 10000)
            if recipe.kw.get("which") == "chroma":
                assert kw["thsadc"] != thsad
                thsad = kw["thsadc"]
            th, s1, s2 = vf.scaled_thresholds(ad, thsad, kw.get("thscd1", 400), kw.get("thscd2", 130))
            assert _usable(oracle, ad, blob, s1, s2) == 1, "the blob is a scene change: its SADs would not be read (blob %d)" % i
        assert th >= 4
        for v in vf.sad_edge_values(th):
            assert (sad == v).any(), (i, v)
        weights.append(np.vectorize(lambda s: vf.degrain_weight(th, s))(sad))
    if consumer == "degrain":
        w = np.stack(weights)
        nonzero = np.count_nonzero(w, axis=0)
        wsrc = np.array([vf.normalised_weights(list(w[:, y, x]))[0] for y in range(w.shape[1]) for x in range(w.shape[2])]).reshape(w.shape[1:])
        assert np.count_nonzero(nonzero == 0) > 0 and np.count_nonzero(nonzero == 1) > 0
        assert np.array_equal(wsrc == 256, nonzero == 0)


@pytest.mark.parametrize("consumer,case", of("scene_count"))
def test_scene_count_fields(oracle, consumer, case):
    fields, ctx = _fields(oracle, consumer, case)
    kw, recipe = ctx["kw"], case[-1]
    for blob, ad, i in fields:
        _, s1, s2 = vf.scaled_thresholds(ad, 400, kw.get("thscd1", 400), kw.get("thscd2", 130))
        _, sad = vf.records(blob, ad)
        over = recipe.kw.get("over", 0) if recipe.kw.get("only") is None or i in recipe.kw["only"] else 0
        assert sad.size % 256 != 0 and 0 < s2 < sad.size - 1
        assert np.count_nonzero(sad > s1) == s2 + over and (sad.ravel()[-(s2 + over):] == s1 + 1).all()
        assert (sad == s1).any()
        assert _usable(oracle, ad, blob, s1, s2) == (0 if over else 1)
    assert {recipe.kw.get("over", 0)} <= {0, 1}


@pytest.mark.parametrize("consumer,case", of("invalid"))
def test_invalid_fields(oracle, consumer, case):
    fields, ctx = _fields(oracle, consumer, case)
    only = case[-1].kw.get("only")
    for blob, ad, i in fields:
        want = 0 if only is None or i in only else 1
        assert blob[4:8].view(np.int32)[0] == want and _usable(oracle, ad, blob, 1 << 40, 1 << 30) == want


def _occlusion_times(oracle, consumer, case):
    """(fields, context, output times of the case, those of them at which the field has every kind of span in both blobs)"""
    fields, ctx = _fields(oracle, consumer, case)
    kw, nf = ctx["kw"], ctx["nf"]
    (bwb, bw, _), (fwb, fw, _) = fields[1], fields[nf + 1]
    ml = float(kw.get("ml", 100.0))
    if consumer == "blockfps":
        f = oracle.BlockFPS(ctx["sup"], bw, fw, nf, 24, 1, **kw)
        times = {f.map(n)[2] for n in range(f.num_frames)} - {0, 256}
    else:
        fk = dict(kw)
        fps = (24, 1) if fk.pop("fps", None) else None
        f = flow_ref.Flow(bw, fw, nf, 1, bw.nHPadding, bw.nVPadding, fps=fps, **fk)
        times = {f.map(n)[2] for n in range(f.num_frames)} - ({0, 256} if fps else set())
        ml = f.ml
    good = []
    for t in sorted(times):
        ok = True
        for blob, ad, isb, mt in ((bwb, bw, 1, 256 - t), (fwb, fw, 0, t)):
            xy, _ = vf.records(blob, ad)
            vx, vy = xy[:, :, 0], xy[:, :, 1]
            st = vf.occlusion_stats(vx, vy, isb, ad, mt, ml)
            m = flow_ref.occlusion_mask(vx, vy, isb, ml, ad.nPel, ad.nBlkX, ad.nBlkY, mt, ad.nBlkSizeX - ad.nOverlapX, ad.nBlkSizeY - ad.nOverlapY)
            ok = ok and st["max_span"] >= 2 and st["at_last"] > 0 and (st["cut_first"] > 0 if isb else st["empty"] > 0)
            ok = ok and (m == 255).any() and ((m > 0) & (m < 255)).any() and st["saturated"] > 0 and st["partial"] > 0
            xmin, xmax, ymin, ymax = vf.legal_rect(ad)
            assert (vx >= xmin[None, :]).all() and (vx <= xmax[None, :]).all() and (vy >= ymin[:, None]).all() and (vy <= ymax[:, None]).all()
        if ok:
            good.append(t)
    return fields, ctx, sorted(times), good


@pytest.mark.parametrize("consumer,case", of("occlusion"))
def test_occlusion_fields(oracle, consumer, case):
    """At one output time of the case at least, in the backward blob (mask time 256 - t) and in the forward blob (mask time t):
    a span of two or more extra blocks, a value of 255 and a value in 1 .. 254; in the backward blob a span cut at block 0 and a range that
    ends on nBlk - 1.  In the forward blob MaskFun.cpp:113 gives maxb = min(bx + 1 - span, nBlkX - 1) with bx < nBlkX - 1 and span >= 0: that
    min() can never bind, a span of two or more leaves the range empty (maxb < minb = bx), and the last block is reached with span 0 only --
    so there the field must hold empty ranges and a range that ends on nBlk - 1."""
    fields, ctx, times, good = _occlusion_times(oracle, consumer, case)
    assert good, "at none of the output times %s the field has every kind of span" % times
    for blob, ad, i in fields:
        _sad_masks_saturate_and_not(consumer, ctx, vf.records(blob, ad)[1], ad)
    if consumer == "flowinter":
        _upsizer_clamps_both_ways(fields, ctx, consumer)


def test_occlusion_cases_lie_on_both_sides_of_the_middle(oracle):
    """together the BlockFPS cases hold good output times below and above time256 128, the flow cases 128 itself and another"""
    sides = set()
    for consumer, case in ALL:
        if case[-1].name == "occlusion":
            sides.update((consumer, "below" if t < 128 else "above" if t > 128 else "at") for t in _occlusion_times(oracle, consumer, case)[3])
    assert {("blockfps", "below"), ("blockfps", "above"), ("flowinter", "at")} <= sides and sides & {("flowinter", "below"), ("flowinter", "above")}, sides


def _oracle_consumers_on_limits(oracle):
    """one run of the oracle's Degrain, Compensate, BlockFPS and Recalculate over `limits` fields (206x118, blk 8/4, pel 2)"""
    import pipeline as pl
    w, h, bits, nf = 206, 118, 8, 3
    frames = pl.moving_clip(w, h, bits, nf, seed=5, noise=3)
    sup = oracle.Super(w, h, bits)
    sf = [sup.frame(f) for f in frames]
    akw = dict(blksize=8, overlap=4)
    bw, fw = oracle.Analyse(sup, isb=1, num_frames=nf, **akw), oracle.Analyse(sup, isb=0, num_frames=nf, **akw)
    bbw = [vf.limits(bw.frame(sf[n], sf[n + 1] if n + 1 < nf else None), bw.ad, 1 + n) for n in range(nf)]
    bfw = [vf.limits(fw.frame(sf[n], sf[n - 1] if n >= 1 else None), fw.ad, 11 + n) for n in range(nf)]
    out = [oracle.Degrain(1, sup, bw.ad).frame(frames[1], [sf[2], sf[0]], [bbw[1], bfw[1]])]
    out.append(oracle.Compensate(sup, bw.ad).frame(sf[0], sf[1], bbw[0]))
    for mode in (0, 3, 5, 8):
        f = oracle.BlockFPS(sup, bw.ad, fw.ad, nf, 24, 1, num=60, den=1, mode=mode)
        out += [f.frame(n, frames, sf, bbw, bfw) for n in range(f.num_frames)]
    for rkw in (dict(blksize=16, overlap=8, smooth=1), dict(blksize=4, overlap=2, smooth=0), dict(blksize=16, overlap=8, smooth=0), dict(blksize=4, overlap=2, smooth=1)):
        oracle.Recalculate(sup, bw.ad, thsad=100, **rkw).frame(sf[0], sf[1], bbw[0])
    return sum(int(p.sum()) for fr in out for p in fr)


def test_oracle_reads_limits_fields_inside_its_frames(tmp_path, oracle):
    """The oracle rebuilt under host AddressSanitizer (CPU code only) runs its four consumers over `limits` fields without a report: a
    block on the limit of its rectangle is fetched from inside the padded planes, so the GPU cases compare against defined samples."""
    rt = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt):
        pytest.skip("gcc has no address sanitizer runtime here")
    odir = os.path.join(ROOT, "oracle")
    so = str(tmp_path / "libmvoracle_asan.so")
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-mavx2", "-fPIC", "-ffp-contract=off", "-fno-strict-aliasing", "-fsanitize=address", "-fno-omit-frame-pointer",
                           "-shared", "-o", so] + [os.path.join(odir, f) for f in ("mvo_super.c", "mvo_analyse.c", "mvo_degrain.c", "mvo_blockfps.c")] + ["-lm"])
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", PYTHONPATH=os.pathsep.join([odir, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), so], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stdout[-1500:] + r.stderr[-4000:]
    assert int(r.stdout.split()[-1]) == _oracle_consumers_on_limits(oracle), "the sanitized build computes something else"


if __name__ == "__main__":   # the child of test_oracle_reads_limits_fields_inside_its_frames: the oracle from the library named on the command line
    import mvoracle
    mvoracle.build = lambda force=False: sys.argv[1]
    mvoracle.lib()
    print(_oracle_consumers_on_limits(mvoracle))
