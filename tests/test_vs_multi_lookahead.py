"""mv.AnalyseN's look-ahead windows, and mv.DegrainN / mv.CompensateN behind them, through the VapourSynth shell (vsplugin/mvtools_vs.c;
MVX_VS_MULTI_LOOKAHEAD = frames per window, 0 = one call per frame).

Whole graphs evaluated through getFrame by one mini-host process per run (the Graph class of tests/test_vs_multi_shell.py).  Every expected byte comes from the
CPU oracle alone (tests/multi_oracle.py, oracle.Analyse / oracle.Degrain / oracle.Compensate), shared between the cases and never changed; what a window run may
differ in is only how the same searches are grouped into launches, so the bytes are the per-frame path's, whatever the window length, the order of the requests
or their number at a time.  The counters come from the line MVX_VS_STATS=1 adds when a window was launched:
    mvtools_vs: AnalyseN windows=W frames=F chains=C largest_window=L
(A device-side hand-over of the multi blobs to the consumers was built with counters of its own, measured and taken out: DESIGN.md 4.3.2.)
The clips are 96x64, the smallest the other shell tests use: several blocks per row, an odd number of block rows."""
import numpy as np
import pytest

import multi_cases as mc
import multi_oracle as mu
import mvoracle as mo
import pipeline as pl
import vs_multi_cases as vc
from test_vs_multi_shell import Graph, _fields_equal, _same, multi_on  # noqa: F401  (multi_on is a fixture)

pytestmark = pytest.mark.gpu

LINE = "mvtools_vs: AnalyseN "


def counters(r):
    """the AnalyseN line of a run's stderr as a dict, or None where it was not printed"""
    lines = [l for l in r.stderr.splitlines() if l.startswith(LINE)]
    assert len(lines) <= 1, r.stderr
    if not lines:
        return None
    out = {k: int(v) for k, v in (t.split("=") for t in lines[0][len(LINE):].split())}
    assert list(out) == ["windows", "frames", "chains", "largest_window"], lines[0]
    return out


def env(length, **more):
    e = {"MVX_VS_STATS": "1", "MVX_VS_MULTI_LOOKAHEAD": str(length)}
    e.update({k: str(v) for k, v in more.items()})
    return e


def first_clip():
    """4:2:0, 8 bits, pel 2, blocks 8 / 4, radius 2, 11 frames: windows of 4 are 4 + 4 + 3 frames, windows of 5 are 5 + 5 + 1"""
    return mu.multi("420", 8, dict(pel=2), vc.B84, 2, nframes=11, fmt_kw=vc.FORMATS["420"])


def check_vectors(g, m, ads, blobs, e, *extra, margs=None, what="multianalyse"):
    """one run that dumps field by field and one that dumps the whole property, both against (ads, blobs); -> the counters of the first"""
    r, path = g.run("multianalyse", *g.cli(margs, None, None, *extra), env=e)
    stride = (blobs[0][0].size + 255) // 256 * 256
    assert r.stdout.splitlines()[0] == "multi radius=%d stride=%d" % (m.radius, stride)
    _fields_equal(mu.fields_of_dump(open(path, "rb").read(), m.n, 2 * m.radius), ads, blobs, what)
    _, path = g.run("multianalyse", *g.cli(margs, None, None, "x.dump=prop", *extra), name="prop.raw", env=e)
    prop = np.fromfile(path, dtype=np.uint8).reshape(m.n, 2 * m.radius, stride)
    for n in range(m.n):
        for f in range(2 * m.radius):
            size = blobs[n][f].size
            assert size < stride
            assert np.array_equal(prop[n, f, :size], blobs[n][f]) and not prop[n, f, size:].any(), (what, n, f)   # the fields at their strides, every pad byte 0
    return counters(r)


# ---------------------------------------------------------------------------------------------------- window runs

@pytest.mark.parametrize("length", [0, 1, 4, 5, 128])
def test_every_window_length_gives_the_oracles_fields(multi_on, oracle, tmp_path, length):
    m = first_clip()
    c = check_vectors(Graph(m, tmp_path), m, m.ads, m.blobs, env(length))
    if length == 0:
        assert c is None   # the per-frame path launches no window: no line
        return
    nw = -(-m.n // length)
    # in order and one request at a time every window is launched exactly once: the first request starts its own, the next one the windows ahead
    assert c == dict(windows=nw, frames=m.n, chains=m.n * 2 * m.radius, largest_window=min(length, m.n))
    if length == 4:
        assert (c["windows"], c["largest_window"], c["chains"]) == (3, 4, 44)
    if length == 128:
        assert c["windows"] == 1


OTHER = {"radius7-above-the-window": vc.ANALYSE_CASES[2], "16bit": vc.ANALYSE_CASES[4], "444": vc.ANALYSE_CASES[5], "gray": vc.ANALYSE_CASES[6], "divide": vc.ANALYSE_CASES[3]}


@pytest.mark.parametrize("name", list(OTHER))
def test_windows_of_four_on_the_other_clips(multi_on, oracle, tmp_path, name):
    case = OTHER[name]
    m = vc.analyse_multi(case)
    assert (name == "radius7-above-the-window") == (m.radius > 4) and (name != "divide" or case[3].get("divide") == 1)
    c = check_vectors(Graph(m, tmp_path), m, m.ads, m.blobs, env(4))
    assert c["windows"] == -(-m.n // 4) and c["frames"] == m.n and c["chains"] == m.n * 2 * m.radius and c["largest_window"] == 4


@pytest.mark.parametrize("extra", [("x.threads=4",), ("x.order=reverse",), ("x.cache=2",)], ids=lambda e: e[0][2:])
def test_order_and_concurrency_do_not_change_a_byte(multi_on, oracle, tmp_path, extra):
    m = first_clip()
    c = check_vectors(Graph(m, tmp_path), m, m.ads, m.blobs, env(4), *extra)
    assert c["windows"] >= 3 and c["frames"] >= m.n   # (a window whose slot was recycled, or whose frames the host dropped, is searched again)


def test_requests_that_find_no_slot_take_the_gated_per_frame_path(multi_on, oracle, tmp_path):
    """windows of ONE frame and eight threads: eleven windows want six slots at once, so some requests find theirs taken and are served by a call of their own,
    behind the admission gate (two at a time here) -- the same bytes, and nothing waits for long"""
    m = first_clip()
    c = check_vectors(Graph(m, tmp_path), m, m.ads, m.blobs, env(1, MVX_VS_MAX_INFLIGHT=2), "x.threads=8")
    assert c["windows"] >= 1 and c["largest_window"] == 1   # (how many requests find a slot depends on how the threads interleave)


# ---------------------------------------------------------------------------------------------------- fields=1

_fields_clip = []


def fields_clip():
    """the first clip's geometry over the (3, -1)-per-frame texture of the shell's own fields test: on the (1, 0) texture of the other cases the half-sample
    vertical shift of a field pair changes no vector, and a shell that dropped the shift would pass"""
    if not _fields_clip:
        frames = pl.moving_clip(mc.W, mc.H, 8, 11, seed=36, noise=3)
        _fields_clip.append(mu.Multi("420", 8, dict(pel=2), vc.B84, 2, frames=frames, fmt_kw=vc.FORMATS["420"]))
    return _fields_clip[0]


def fields_expected(m, order):
    """oracle.Analyse(fields=1) of every (frame, field) with the shift of the frames' parities (_Field = order ^ (n % 2), as x.fieldorder sets it)"""
    ads, blobs, shifts = [], [[] for _ in range(m.n)], set()
    for r in range(2 * m.radius):
        isb, delta = mc.field_of(r)
        an = mo.Analyse(m.osup, num_frames=m.n, isb=isb, delta=delta, fields=1, **m.akw)
        ads.append(an.ad)
        for n in range(m.n):
            nref = m.nref(n, r)
            fs = 0
            if nref is not None:
                fs, miss = mo.field_shift(1, m.osup.s.pel, n, nref, src_field=order ^ (n % 2), ref_field=order ^ (nref % 2))
                assert not miss
                shifts.add((delta % 2, fs))
            blobs[n].append(an.frame(m.osf[n], m.ref(n, r), field_shift=fs))
    return ads, blobs, shifts


def test_fields_take_their_shift_from_the_source_frames(multi_on, oracle, tmp_path):
    m = fields_clip()
    assert m.osup.s.pel == 2
    ads, blobs, shifts = fields_expected(m, 0)
    assert shifts == {(1, 1), (1, -1), (0, 0)}   # both signs at the odd distance, none at the even one
    assert any(not np.array_equal(blobs[n][0], m.blobs[n][0]) for n in range(m.n))   # and the shift changes vectors
    c = check_vectors(Graph(m, tmp_path), m, ads, blobs, env(4), "x.fieldorder=0", margs=dict(fields=1), what="fields=1")
    assert c["windows"] == 3


def test_fields_without_parity_information_fail_in_the_reference_words(multi_on, tmp_path):
    m = fields_clip()
    g = Graph(m, tmp_path)
    r, _ = g.run("multianalyse", *g.cli(dict(fields=1)), env=env(4), check=False)
    assert "AnalyseN: _Field property not found in input frame. Therefore, you must pass tff argument." in r.stdout, r.stdout + r.stderr
    r, _ = g.run("multianalyse", *g.cli(dict(fields=1, tff=1)), env=env(4))
    assert counters(r)["windows"] == 3


# ---------------------------------------------------------------------------------------------------- consumers behind windows of two

DEGRAIN = vc.DEGRAIN_CASES[2]          # 204x116, 16 bits, blocks 16 / 8, radius 3, 7 frames, oracle.Degrain
COMPENSATE = vc.COMPENSATE_CASES[1]    # 96x64, 8 bits, blocks 8 / 4, tr 3, 9 frames, oracle.Compensate
THREADS = {1: (), 4: ("x.threads=4", "x.order=frame")}


@pytest.mark.parametrize("threads", [1, 4])
def test_multidegrain_through_windows_of_two(multi_on, oracle, tmp_path, threads):
    assert DEGRAIN[6] == 3 and DEGRAIN[7] == "oracle"
    m = vc.degrain_multi(DEGRAIN)
    g = Graph(m, tmp_path)
    want = vc.degrain_expected(oracle, DEGRAIN, frames=range(m.n))
    r, path = g.run("multidegrain", *g.cli(None, None, DEGRAIN[8], *THREADS[threads]), env=env(2))
    _same(g.read(path, m.n), want, "DegrainN")
    c = counters(r)
    assert c["windows"] >= -(-m.n // 2) and c["largest_window"] == 2


@pytest.mark.parametrize("threads", [1, 4])
def test_multicompensate_through_windows_of_two(multi_on, oracle, tmp_path, threads):
    m = vc.compensate_multi(COMPENSATE)
    tr = vc.compensate_tr(COMPENSATE)
    assert tr == 3
    g = Graph(m, tmp_path)
    want = vc.compensate_expected(oracle, COMPENSATE)
    r, path = g.run("multicompensate", *g.cli(None, None, COMPENSATE[5], *THREADS[threads]), env=env(2))
    assert "permits out" not in r.stderr, r.stderr
    _same(g.read(path, m.n * (2 * tr + 1)), want, "CompensateN")
    c = counters(r)
    assert c["windows"] >= -(-m.n // 2) and c["largest_window"] == 2


def test_more_windows_than_slots_last_to_first(multi_on, oracle, tmp_path):
    """15 frames in windows of 2 are 8 windows on 6 slots, asked for last to first: creation reads frame 0 (window 0), window 6 takes its slot, and frame 1 starts
    window 0 a second time -- every frame is the oracle's whichever launch made it"""
    radius = 3
    m = mu.multi("420", 8, dict(pel=2), vc.B84, radius, nframes=15, fmt_kw=vc.FORMATS["420"])
    g = Graph(m, tmp_path)
    dg = mo.Degrain(radius, m.osup, m.ads[0])
    want = [dg.frame(m.frames[n], [m.ref(n, r) for r in range(2 * radius)], m.blobs[n]) for n in range(m.n)]
    r, path = g.run("multidegrain", *g.cli(None, None, None, "x.order=reverse"), env=env(2))
    _same(g.read(path, m.n), want, "DegrainN")
    c = counters(r)
    assert c["windows"] >= 9 and c["frames"] >= m.n + 2, c   # windows 0 .. 7, and window 0 again
