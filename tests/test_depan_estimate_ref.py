"""CPU tests of the restatement of mv.DepanEstimate (tests/depan_estimate_ref.py) and of the cases every other DepanEstimate test stands on
(tests/depan_estimate_cases.py): creation as in MVDepan.cpp:1271-1433 with the library's refusals, each case held to what it claims with the
margins that make its discrete results independent of the FFT, and stage 3 against a table written by hand."""
import numpy as np
import pytest

import depan_estimate_cases as dc
import depan_estimate_ref as er

f32 = np.float32


def _err(**kw):
    with pytest.raises(er.CreateError) as e:
        er.Estimate(kw.pop("w", 640), kw.pop("h", 480), **kw)
    return str(e.value)


def test_defaults_and_automatic_windows():
    e = er.Estimate(1920, 1080)
    assert (e.winx, e.winy, e.wleft, e.wtop, e.dxmax, e.dymax, e.windows) == (1024, 1024, 448, 28, 256, 256, 1)
    assert (e.trust_limit, e.zoommax, e.stab, e.pixaspect) == (4, 1, 1, 1) and e.spectrum_bytes == 1024 * 513 * 8
    e = er.Estimate(3840, 2160, 16)
    assert (e.winx, e.winy, e.wleft, e.wtop, e.dxmax, e.dymax) == (2048, 2048, 896, 56, 512, 512)
    e = er.Estimate(64, 48)
    assert (e.winx, e.winy, e.wleft, e.wtop, e.dxmax, e.dymax) == (64, 32, 0, 8, 16, 8)
    # zoom: winx halves and both windows are centred in their halves
    e = er.Estimate(1920, 1080, zoommax=1.5)
    assert (e.winx, e.winy, e.wleft, e.wtop, e.dxmax, e.windows) == (512, 1024, 224, 28, 128, 2)
    e = er.Estimate(1920, 1080, zoommax=1.5, winx=512, wleft=100, wtop=9, winy=64)
    assert (e.winx, e.winy, e.wleft, e.wtop) == (256, 64, 100, 9)
    assert er.auto_window(8192) == 8192 and er.auto_window(20000) == 8192 and er.auto_window(8191) == 4096 and er.auto_window(1) == 1


def test_error_texts_in_the_reference_order_then_the_refusals():
    T, P = "DepanEstimate: trust must be between 0.0 and 100.0 (inclusive).", "DepanEstimate: pixaspect must be positive."
    F = "DepanEstimate: clip must have constant format and dimensions, it must be YUV or Gray, and it must be 8..16 bit integer or 32 bit float."
    WX, WY = "DepanEstimate: winx must not be greater than width-wleft.", "DepanEstimate: winy must not be greater than height-wtop."
    DX, DY = "DepanEstimate: dxmax must be less than winx/2.", "DepanEstimate: dymax must be less than winy/2."
    assert _err(trust=-0.5) == T and _err(trust=100.5) == T
    assert _err(pixaspect=0.0) == P
    assert _err(bits=17) == F and _err(bits=16, float_samples=True) == F
    assert _err(winx=1024) == WX and _err(winx=512, wleft=200) == WX
    assert _err(winy=512) == WY and _err(winy=256, wtop=300) == WY
    assert _err(winx=64, dxmax=32) == DX and _err(winy=64, dymax=32) == DY
    bad = dict(trust=101, pixaspect=-1, bits=17, winx=1024, winy=512, dxmax=9999, dymax=9999)
    for text in (T, P, F, WX, WY, DX, DY):
        assert _err(**bad) == text
        bad.pop(next(iter(bad)))
    # the limits pass
    er.Estimate(640, 480, trust=0.0), er.Estimate(640, 480, trust=100.0), er.Estimate(640, 480, winx=64, winy=64, dxmax=31, dymax=31)
    # the library's refusals come after the reference's own checks
    assert _err(bits=32, float_samples=True) == "DepanEstimate: float clips are not supported."
    assert _err(bits=32, float_samples=True, dxmax=9999) == DX
    POW = "DepanEstimate: winx (after the halving for zoom) and winy must be powers of two between 8 and 8192."
    assert _err(winx=100) == POW and _err(winy=48) == POW and _err(winx=4, winy=8) == POW
    assert _err(winx=24, zoommax=1.2) == POW and _err(w=4, h=4) == POW     # 12 after the halving; automatic 4 x 4
    assert _err(w=20000, h=64, winx=16384) == POW
    er.Estimate(20000, 64)                                                # the automatic size stops at 8192
    assert _err(zoommax=1.2, winx=256, wleft=200) == "DepanEstimate: every window must lie inside the frame."   # 200 + 320 + 128 > 640


def _area(e, surface):
    rows = list(range(0, e.dymax + 1)) + list(range(e.winy - e.dymax, e.winy))
    cols = list(range(0, e.dxmax + 1)) + list(range(e.winx - e.dxmax, e.winx))
    return rows, cols, surface[np.ix_(rows, cols)].astype(np.float64)


def _want(c, e):
    """the planted pan as the filter reports it"""
    px = c.pan[0] if c.pan2 is None else (c.pan[0] + c.pan2[0]) / 2
    py = c.pan[1] if c.pan2 is None else (c.pan[1] + c.pan2[1]) / 2
    if e.fields:
        py = 2 * py + (1 if e.top_field(c.n, c.prop) else -1)
    return px, py / float(e.pixaspect)


@pytest.mark.parametrize("c", dc.CASES, ids=repr)
def test_every_case_holds_its_claim(c):
    e, a, b = c.ref(), c.result(64), c.result(32)
    apart = lambda v, edge, m: abs(float(v) - edge) > m
    mts = []
    for w in range(e.windows):
        s64, s32, A, B = a["surfaces"][w], b["surfaces"][w], a["scans"][w], b["scans"][w]
        da, db = a["dbg"][w], b["dbg"][w]
        # the peak leads every other candidate by 1000 times what the two FFTs differ by, so any FFT of that quality finds it
        assert (A["imax"], A["jmax"]) == (B["imax"], B["jmax"])
        rows, cols, area = _area(e, s64)
        area[rows.index(A["jmax"]), cols.index(A["imax"])] = -np.inf
        differ = float(np.abs(s64.astype(np.float64) - s32.astype(np.float64)).max())
        assert float(A["max"]) - area.max() >= 1000 * differ, (float(A["max"]) - area.max(), differ)
        # the thresholds: 100 times the two runs' difference away (in trust, and in the quantity itself where that is larger; never less than an ulp)
        mt = 100 * max(abs(float(da["trust"]) - float(db["trust"])), float(np.spacing(f32(da["trust"]))))
        mts.append(mt)
        assert apart(da["trust"], float(e.trust_limit), mt)
        assert da["scene_change"] == db["scene_change"] == (c.claim == "scene_change" or (c.claim == "bad_zoom_scene" and w == 1))
        if not da["scene_change"]:
            mx = max(mt, 100 * abs(float(da["raw_fdx"]) - float(db["raw_fdx"])))
            assert apart(abs(da["raw_fdx"]), 0.01, mx)
            assert apart(abs(float(da["dx"]) + float(da["xadd"])), e.dxmax, max(mt, 100 * abs(float(da["xadd"]) - float(db["xadd"]))))
            assert apart(abs(float(da["dy"]) + float(da["yadd"])), e.dymax, max(mt, 100 * abs(float(da["yadd"]) - float(db["yadd"]))))
    if e.windows == 2:
        za, zb = float(a["dbg"][0]["zoom_raw"]), float(b["dbg"][0]["zoom_raw"])
        assert apart(abs(za - 1), float(e.zoommax) - 1, max(max(mts), 100 * abs(za - zb)))
        assert a["good_zoom"] == b["good_zoom"] == (c.claim == "zoom")
    for r in (a, b):
        if c.claim in ("pan", "zoom"):
            px, py = _want(c, e)
            assert abs(float(r["dx"]) - px) <= 0.5 and abs(float(r["dy"]) - py) <= 0.5, (r["dx"], r["dy"], px, py)
        else:
            assert (r["dx"], r["dy"], r["zoom"]) == (0, 0, 1)
        if c.claim == "zoom":
            assert abs(float(r["zoom"]) - (1 + (c.pan2[0] - c.pan[0]) / (c.width // 2))) <= 1.0 / (c.width // 2)
        if c.claim == "frame0":
            assert r["trust"] == 0 and not r["dbg"][0]["scene_change"]      # a good pair, zeroed by the frame-0 rule alone
        if c.claim == "bad_zoom":
            assert not any(d["scene_change"] for d in r["dbg"])            # both windows found their pan: the zoom alone is refused


def test_the_cases_cover_the_windows_and_paths_they_name():
    sizes = {(c.ref().winx, c.ref().winy, c.bits) for c in dc.CASES}
    for wx, wy in dc.WINDOWS:
        assert (wx, wy, 8) in sizes and (wx, wy, 16) in sizes
    for n in dc.PATH_LENGTHS:
        assert any(s[0] == n for s in sizes) and any(s[1] == n for s in sizes)
    assert any(c.bits == 10 for c in dc.CASES)
    assert any(c.ref().wleft % 2 and c.ref().wtop % 2 for c in dc.CASES)


@pytest.mark.parametrize("nf,n,trusts,zeroed", dc.STAGE3)
def test_stage3_table(nf, n, trusts, zeroed):
    e = er.Estimate(64, 48, trust=4.0, num_frames=nf)
    trio = [dict(dx=1.5, dy=-2.5, zoom=1.01, trust=t) for t in trusts]
    assert e.finish(n, trio) == ((0, 0, 1, 0) if zeroed else (f32(1.5), f32(-2.5), f32(1.01), 0))
