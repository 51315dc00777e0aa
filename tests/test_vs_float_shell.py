"""32-bit float clips through the VapourSynth filter shell (vsplugin/mvtools_vs.c) with MVX_VS_FLOAT=1 in the host's environment as the plugin is loaded.

The switch registers nothing: it widens what mv.Super and the filters with a float entry in the library accept (Compensate, BlockFPS; with MVX_VS_MULTI=1 DegrainN
and CompensateN; with MVX_VS_FLOW=1 FlowInter, FlowFPS, Flow, FlowBlur; with MVX_VS_DEPAN=1 DepanCompensate and DepanStabilise).  Every other filter refuses a float
clip or a float super clip, and without the switch every message is what it was.

CPU part: the function lists, and what creation alone decides -- through the mini host's `list` and `error`, which touch no device.  No test here puts a library in
front of the plugin, so everything that needs a frame (frame 0 of a super or vector clip included) is a GPU test.

GPU part: one mini-host process per case, each under its own time limit.  The float clip is degrain_float_cases.float_clip of the integer clip (`x.float=`), the
final filter gets it and a second mv.Super built on it, the vectors and the Depan data come from the integer clip.  Expected planes come from the numpy restatements
fed the Super restatement's frames and the CPU oracle's search (tests/vs_float_cases.py) -- never from the shell, the Python package or the library -- and are
compared as uint32, bit for bit: the shell only moves bytes around kernels that are exact already.

mv.DepanAnalyse and mv.SCDetection are not among the refusals: they read no sample of their clip (they copy its frames and attach properties), take a float clip
today as the reference does, and keep doing so with and without the switch; a GPU case holds that the frames come out bit for bit.

The Depan cases run on tests/test_vs_depan_shell.py's panning clip at three shapes: its own 128x96 4:2:0, whose float rows fill the 256-byte device pitch exactly, and
70x54 4:4:4 and 100x72 4:2:2, whose rows do not."""
import subprocess

import numpy as np
import pytest

import degrain_float_cases as fc
import depan_float_ref as dfr
import depan_ref as dr
import depan_stab_ref as sr
import pipeline as pl
import super_float_ref as sf
import test_vs_shim as shim
import vs_float_cases as vc
from test_vs_shim import host

gpu = pytest.mark.gpu
SWITCHES = ("MVX_VS_FLOW", "MVX_VS_DEPAN", "MVX_VS_MULTI", "MVX_VS_FLOAT", "MVX_VS_MASK_DEEP")
FORMAT_MSG = "%s: input clip must be GRAY, 420, 422, 440, or 444, up to 16 bits, with constant dimensions."
DEPAN_FORMAT_MSG = "%s: clip must have constant format and dimensions, integer sample type, bit depth up to 16, and it must be Gray, 420, 422, or 444, and not RGB."


@pytest.fixture
def plain(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


@pytest.fixture
def float_on(monkeypatch, plain):
    monkeypatch.setenv("MVX_VS_FLOAT", "1")   # (proc_env() copies os.environ)


def _listed():
    out = host("list").splitlines()
    assert out[0] == "id=com.nodame.mvtools ns=mv"
    return dict(line.split(" ", 1) for line in out[1:])


def _error(*args):
    return host("error", *args).strip()


# ---------------------------------------------------------------------------------------------------- CPU: the function lists

def test_the_switch_registers_nothing(monkeypatch, plain):
    assert _listed() == shim.EXPECTED
    for v in ("1", "0"):
        monkeypatch.setenv("MVX_VS_FLOAT", v)
        assert _listed() == shim.EXPECTED


@pytest.mark.parametrize("other", SWITCHES[:3])
def test_the_switch_changes_no_other_switchs_list(monkeypatch, plain, other):
    monkeypatch.setenv(other, "1")
    without = _listed()
    assert len(without) > len(shim.EXPECTED)
    monkeypatch.setenv("MVX_VS_FLOAT", "1")
    assert _listed() == without


# ---------------------------------------------------------------------------------------------------- CPU: mv.Super at creation

SUPER_FORMATS = [("420", 70, 54, {}), ("422", 70, 54, dict(pel=4)), ("444", 140, 38, dict(hpad=8, vpad=4)), ("gray", 36, 36, dict(hpad=0, vpad=0, pel=1))]


@pytest.mark.parametrize("fmt,w,h,skw", SUPER_FORMATS, ids=[c[0] for c in SUPER_FORMATS])
def test_super_on_a_float_clip_is_a_float_clip_of_the_super_clips_size(float_on, fmt, w, h, skw):
    i = vc.info_of(skw)
    sub = (1, 1) if fmt == "gray" else vc.SUB[fmt]
    (sh, sw), = sf.geometry(w, h, sub, fmt == "gray", i.hpad, i.vpad, i.pel)[1][:1]
    got = _error("Super", w, h, 16, "x.float=clip", "x.format=" + fmt, *vc.cli("f", skw))
    ssw, ssh = (0, 0) if fmt == "gray" else sub
    assert got == "OK %dx%d frames=4 sample=float bits=32 ssw=%d ssh=%d planes=%d" % (sw, sh, ssw, ssh, 1 if fmt == "gray" else 3)


@pytest.mark.parametrize("fmt", ["420", "422", "444", "gray"])
def test_without_the_switch_super_refuses_a_float_clip_in_todays_words(monkeypatch, plain, fmt):
    for v in (None, "0"):
        if v:
            monkeypatch.setenv("MVX_VS_FLOAT", v)
        assert _error("Super", 70, 54, 16, "x.float=clip", "x.format=" + fmt) == "ERROR " + FORMAT_MSG % "Super"
        assert _error("Super", 70, 54, 16, "x.float=clip", "x.format=" + fmt, "f.levels=2") == "ERROR " + FORMAT_MSG % "Super"
        assert _error("Super", 70, 54, 16, "x.float=clip", "x.format=" + fmt, "f.pel=3") == "ERROR Super: pel must be 1, 2, or 4."   # (argument values first, as now)


PEL = ["x.pelw=140", "x.pelh=108"]


@pytest.mark.parametrize("args,msg", [
    # the library's order: levels, then pel / sharp / rfilter, then the format, then the padding; the shell's pelclip message where the pelclip's own checks sit
    (("f.levels=2",), "Super: a float super clip has one level (levels=1)."),
    (("f.levels=0",), "Super: a float super clip has one level (levels=1)."),
    (("f.levels=2", "f.pel=3"), "Super: a float super clip has one level (levels=1)."),
    (("f.pel=3",), "Super: pel must be 1, 2, or 4."),
    (("f.pel=3", "f.hpad=-1", *PEL), "Super: pel must be 1, 2, or 4."),
    (("f.sharp=3", "f.hpad=-1"), "Super: sharp must be between 0 and 2 (inclusive)."),
    (("f.hpad=-1", *PEL), "Super: hpad and vpad must not be negative."),
    (PEL, "Super: pelclip is not supported on float clips."),
    (("x.pelw=100", "x.pelh=100"), "Super: pelclip is not supported on float clips."),   # (whatever its size)
])
def test_super_messages_come_in_their_order(float_on, args, msg):
    assert _error("Super", 70, 54, 16, "x.float=clip", *args) == "ERROR " + msg
    assert _error("Super", 70, 54, 16, "x.float=clip", "f.levels=1").startswith("OK ")


def test_a_float_clip_at_subsampling_2_is_refused_after_levels_and_pel(monkeypatch, float_on):
    """x.format=410: subsampling 2 in both directions.  The library's format message, after its levels and pel messages and before the padding's"""
    sub2 = ("Super", 72, 56, 16, "x.float=clip", "x.format=410")
    assert _error(*sub2, "f.levels=2", "f.pel=3") == "ERROR Super: a float super clip has one level (levels=1)."
    assert _error(*sub2, "f.pel=3") == "ERROR Super: pel must be 1, 2, or 4."
    assert _error(*sub2, "f.hpad=-1") == "ERROR " + FORMAT_MSG % "Super"
    assert _error(*sub2, *PEL) == "ERROR " + FORMAT_MSG % "Super"
    monkeypatch.setenv("MVX_VS_FLOAT", "0")
    assert _error(*sub2) == "ERROR " + FORMAT_MSG % "Super"
    assert _error("Super", 72, 56, 16, "x.format=410") == "ERROR " + FORMAT_MSG % "Super"   # (as an integer clip of that format)


# ---------------------------------------------------------------------------------------------------- CPU: the other filters at creation

def test_finest_and_analyse_refuse_a_float_super_clip_in_the_librarys_words(float_on):
    # (x.fakesuper=1: a blank float clip of the float super clip's size with its Super_* properties on frame 0 -- creation reads nothing else, and no device is needed)
    for fmt in ("420", "gray"):
        assert _error("Finest", 70, 54, 16, "x.float=super", "x.fakesuper=1", "x.format=" + fmt) == "ERROR Finest: float super clips are not supported."
        assert _error("Analyse", 70, 54, 16, "x.float=super", "x.fakesuper=1", "x.format=" + fmt) == "ERROR Analyse: float super clips are not supported."


def test_finests_refusal_in_the_shell_is_the_librarys_text():
    """mv.Finest refuses a float super clip at creation, where the library's mvx_finest_frames would refuse it at the first frame: one text in both places"""
    import os
    msg = '"Finest: float super clips are not supported."'
    for path in ("csrc/mvx_super.hip", "vsplugin/mvtools_vs.c"):
        with open(os.path.join(shim.PKG, path)) as f:
            assert msg in f.read(), path


def test_analysen_refuses_a_float_super_clip_in_the_librarys_words(monkeypatch, float_on):
    monkeypatch.setenv("MVX_VS_MULTI", "1")
    assert _error("AnalyseN", 70, 54, 16, "x.float=super", "x.fakesuper=1", "f.radius=2") == "ERROR AnalyseN: float super clips are not supported."


@pytest.mark.parametrize("filt", ["DepanCompensate", "DepanStabilise"])
def test_the_depan_warps_take_a_float_clip_with_the_switch_only(monkeypatch, plain, filt):
    monkeypatch.setenv("MVX_VS_DEPAN", "1")
    extra = ("f.offset=1.0",) if filt == "DepanCompensate" else ()
    assert _error(filt, 70, 54, 8, "x.float=clip", *extra) == "ERROR " + DEPAN_FORMAT_MSG % filt
    monkeypatch.setenv("MVX_VS_FLOAT", "1")
    for fmt, planes, ss in (("420", 3, 1), ("444", 3, 0), ("gray", 1, 0)):
        assert _error(filt, 70, 54, 8, "x.float=clip", "x.format=" + fmt, *extra) == "OK 70x54 frames=4 sample=float bits=32 ssw=%d ssh=%d planes=%d" % (ss, ss, planes)
    # the library's checks and messages are the integer entry's, in its order
    bad = ("f.offset=11.0", "DepanCompensate: offset must be between -10.0 and 10.0 (inclusive).") if filt == "DepanCompensate" else ("f.method=2", "DepanStabilise: method must be between 0 and 1 (inclusive).")
    assert _error(filt, 70, 54, 8, "x.float=clip", bad[0]) == "ERROR " + bad[1]


def test_depanestimate_refuses_a_float_clip_with_and_without_the_switch(monkeypatch, plain):
    monkeypatch.setenv("MVX_VS_DEPAN", "1")
    assert _error("DepanEstimate", 128, 96, 8, "x.float=clip") == "ERROR DepanEstimate: float clips are not supported."
    monkeypatch.setenv("MVX_VS_FLOAT", "1")
    assert _error("DepanEstimate", 128, 96, 8, "x.float=clip") == "ERROR DepanEstimate: float clips are not supported."


def test_invocations_without_the_new_arguments_print_what_they_printed(float_on):
    assert _error("Super", 640, 360, 8, "f.pel=1") == "OK 672x978 frames=4"


# ---------------------------------------------------------------------------------------------------- CPU: the cases with parameters of their own test what they claim

def test_the_plane0_limit2_case_limits_luma_and_leaves_chroma(oracle):
    name = "A-r3-16/8-plane0-limit2"
    q, floats = vc.degrain_clip(name)
    want, refs = vc.degrain_expected(oracle, name, q, floats, [3])
    w = refs[3].plan[0][1]
    assert np.count_nonzero(w) and len(np.unique(w[w > 0])) > 3, "the weights do not differ per block"
    case = vc.DEGRAIN_CASES[name]
    vc.DEGRAIN_CASES["unlimited"] = case[:6] + (dict(plane=0),)
    try:
        free, _ = vc.degrain_expected(oracle, "unlimited", q, floats, [3])
    finally:
        del vc.DEGRAIN_CASES["unlimited"]
    lim = np.float32(2) / np.float32(255)
    moved = np.abs(free[3][0] - floats[3][0])
    assert float((moved > lim).mean()) > 0.01, "the limit binds nowhere"                      # the unlimited filter moves samples further than the limit ...
    # ... and the limited one does not: src +- L is rounded once and the difference once more, on values below 2 (an ulp of 2^-23 at the most)
    assert float(np.abs(want[3][0] - floats[3][0]).max()) <= float(lim) + 2.0 ** -22
    assert not np.array_equal(vc.bits(want[3][0]), vc.bits(free[3][0])) and not np.array_equal(vc.bits(want[3][0]), vc.bits(floats[3][0]))
    for p in (1, 2):
        assert np.array_equal(vc.bits(want[3][p]), vc.bits(floats[3][p]))


def test_the_scene_case_has_a_scene_change_on_one_side_only(oracle):
    name = "A-r3-8/4-scene"
    q, floats = vc.degrain_clip(name)
    want, refs = vc.degrain_expected(oracle, name, q, floats, [3, 4])
    w = refs[3].plan[0][1]   # frame 3: the backward references 4, 5, 6 lie behind the cut
    assert not np.any(w[:, [0, 2, 4]]) and np.count_nonzero(w[:, [1, 3, 5]]) and len(np.unique(w[w > 0])) > 3
    w = refs[4].plan[0][1]   # frame 4: the forward references 3, 2, 1 lie before it
    assert not np.any(w[:, [1, 3, 5]]) and np.count_nonzero(w[:, [0, 2]])
    assert not np.array_equal(vc.bits(want[3][0]), vc.bits(floats[3][0]))


def test_the_mode0_blockfps_case_interpolates(oracle):
    case = vc.FPS_CASES["70x54-mode0"]
    q, floats = vc.fps_clip(case)
    want, times = vc.fps_expected(oracle, case, q, floats)
    assert len(want) == 11 and times.count(0) == 3
    for n, t in enumerate(times):
        copies = any(all(np.array_equal(vc.bits(want[n][p]), vc.bits(f[p])) for p in range(3)) for f in floats)
        assert copies == (t == 0), (n, t)


# ---------------------------------------------------------------------------------------------------- GPU: Super

def _graph(tmp_path, q, floats, w, h, bits, fmt):
    return vc.Graph(tmp_path, q, floats, w, h, bits, fmt)


@gpu
@pytest.mark.parametrize("case", vc.SUPER_CASES, ids=lambda c: "%dx%d-%s-pel%d-sharp%d-pad%dx%d" % (c[0] + (c[1], c[2], c[3]) + c[4]))
def test_super_frames_are_the_restatements_in_their_defined_rectangles(tmp_path, case):
    size, fmt, pel, sharp, pad = case
    q, floats = vc.super_clip(size, fmt)
    g = _graph(tmp_path, q, floats, size[0], size[1], 16, fmt)
    skw = dict(pel=pel, sharp=sharp, hpad=pad[0], vpad=pad[1])
    r, path = g.run("super", *vc.cli("s", skw))
    shp = vc.super_shapes(size, fmt, pel, pad)
    assert "super %dx%d Super_height=%d Super_hpad=%d Super_vpad=%d Super_pel=%d Super_modeyuv=%d Super_levels=1" % (
        shp[0][1], shp[0][0], size[1], pad[0], pad[1], pel, 1 if fmt == "gray" else 7) in r.stdout
    got = vc.read_float(path, shp, 3)
    for n in range(3):
        want, defined = sf.frame(floats[n], **vc.super_kw(fmt, skw))
        for p in range(len(want)):
            assert want[p].shape == got[n][p].shape
            assert pl.first_diff(np.where(defined[p], got[n][p], 0).view(np.uint32), vc.bits(want[p])) == "", "frame %d plane %d" % (n, p)
            assert not vc.bits(got[n][p])[~defined[p]].any(), "frame %d plane %d: not zero outside the defined rectangles" % (n, p)


# ---------------------------------------------------------------------------------------------------- GPU: DegrainN

def _degrain_cli(name):
    _, fmt, bits, skw, akw, radius, dkw = vc.DEGRAIN_CASES[name]
    return vc.cli("s", skw) + ["m.radius=%d" % radius] + vc.cli("m", akw) + vc.cli("f", dkw)


def _degrain_graph(tmp_path, name):
    (w, h), fmt, bits = vc.DEGRAIN_CASES[name][:3]
    q, floats = vc.degrain_clip(name)
    return _graph(tmp_path, q, floats, w, h, bits, fmt)


def _expect_some(want, n):
    return [want.get(k) for k in range(n)]


@gpu
@pytest.mark.parametrize("name", list(vc.DEGRAIN_CASES))
def test_degrainn_on_a_float_clip_is_the_restatement(oracle, tmp_path, name):
    g = _degrain_graph(tmp_path, name)
    targets = [3, 4] if name.endswith("scene") else [0, g.n // 2, g.n - 1]   # the middle frame, and the clip's ends with their references outside the clip
    want, refs = vc.degrain_expected(oracle, name, g.q, g.floats, targets)
    w = refs[targets[1]].plan[0][1]
    assert np.count_nonzero(w) and len(np.unique(w[w > 0])) > 3, "the weights do not differ per block"
    _, path = g.run("multidegrain", *_degrain_cli(name))
    vc.same(g.read(path), _expect_some(want, g.n), name)


@gpu
def test_degrainn_from_eight_threads_in_reverse_order_is_the_single_threaded_result(oracle, tmp_path):
    name = "A-r3-8/4"
    g = _degrain_graph(tmp_path, name)
    want, _ = vc.degrain_expected(oracle, name, g.q, g.floats, [0, 3, 6])
    _, one = g.run("multidegrain", *_degrain_cli(name), name="one.raw")
    _, many = g.run("multidegrain", *_degrain_cli(name), "x.threads=8", "x.order=frame", "x.threadorder=reverse", name="many.raw")
    vc.same(g.read(one), _expect_some(want, g.n), "one thread")
    vc.same(g.read(many), g.read(one), "eight threads, last frame first")


@gpu
@pytest.mark.parametrize("env", [{}, {"MVX_VS_CACHE_FRAMES": "0"}], ids=["cached", "no-device-cache"])
def test_lazy_super_frames_work_for_a_float_super_clip(oracle, tmp_path, env):
    """MVX_VS_SUPER_LAZY=1 works for a float mv.Super as for an integer one: its host frames carry the source picture, the device copy serves the consumers, and without a
    device cache every consumer rebuilds the float super frame from the embedded source"""
    name = "A-r3-8/4"
    g = _degrain_graph(tmp_path, name)
    want, _ = vc.degrain_expected(oracle, name, g.q, g.floats, [0, 3, 6])
    _, path = g.run("multidegrain", *_degrain_cli(name), env=dict(env, MVX_VS_SUPER_LAZY="1"))
    vc.same(g.read(path), _expect_some(want, g.n), "lazy")
    # ... and the host frames of the lazy float super clip: the source in the corner of a frame of zeros
    r, sup = g.run("super", name="sup.raw", env=dict(env, MVX_VS_SUPER_LAZY="1"))
    got = vc.read_float(sup, vc.super_shapes((g.w, g.h), g.fmt, 2, (16, 16)), g.n)
    for p in range(3):
        h, w = g.floats[0][p].shape
        assert np.array_equal(vc.bits(got[0][p][:h, :w]), vc.bits(g.floats[0][p])) and not vc.bits(got[0][p][h:]).any() and not vc.bits(got[0][p][:, w:]).any()


@gpu
def test_without_a_device_cache_consumers_upload_the_float_super_frames_from_the_host(oracle, tmp_path):
    """MVX_VS_CACHE_FRAMES=0 without the lazy setting: no device copy of a super frame survives its getFrame, so mv.DegrainN uploads every reference from the 4-byte host
    frame mv.Super handed out (super_to_device with 4-byte samples and 256-byte pitches)"""
    name = "A-r3-8/4"
    g = _degrain_graph(tmp_path, name)
    want, _ = vc.degrain_expected(oracle, name, g.q, g.floats, [0, 3, 6])
    _, path = g.run("multidegrain", *_degrain_cli(name), env={"MVX_VS_CACHE_FRAMES": "0"})
    vc.same(g.read(path), _expect_some(want, g.n), "no device cache")


@gpu
def test_a_float_and_an_integer_graph_in_one_process_are_both_right(oracle, tmp_path):
    import degrain_n_cases as dc
    import mvoracle as mo
    name = "A-r1-16/8"
    (w, h), fmt, bits, skw, akw, radius, dkw = vc.DEGRAIN_CASES[name]
    g = _degrain_graph(tmp_path, name)
    want, _ = vc.degrain_expected(oracle, name, g.q, g.floats, [0, 1, 2])
    ipath = tmp_path / "int.raw"
    _, path = g.run("multidegrain", *_degrain_cli(name), "x.intout=%s" % ipath)
    vc.same(g.read(path), _expect_some(want, g.n), "the float graph")
    got = shim._read_frames(ipath, w, h, bits, g.n)
    for t in range(g.n):
        osup, sfr, ad, nrefs, blobs = fc.oracle_job(oracle, g.q, w, h, bits, radius, t, akw, skw)
        iw = mo.Degrain(radius, osup, ad).frame(g.q[t], [sfr[m] if m is not None else None for m in nrefs], blobs)
        for p in range(3):
            assert np.array_equal(got[t][p], iw[p]), "the integer graph: frame %d plane %d: %s" % (t, p, pl.first_diff(got[t][p], iw[p]))
    assert dc.FORMATS[fmt] == {}


# ---------------------------------------------------------------------------------------------------- GPU: Compensate, CompensateN, BlockFPS

@gpu
@pytest.mark.parametrize("name", list(vc.COMP_CASES))
def test_compensate_on_a_float_clip_is_the_restatement(oracle, tmp_path, name):
    case = vc.COMP_CASES[name]
    fmt, bits, blk, tr, w, h, thsad = case
    q, floats = vc.comp_clip(case)
    want, used = vc.compensate_expected(oracle, case, q, floats, 2)
    assert used and 0.3 < min(used) and max(used) < 1.0, used   # compensated blocks and fallbacks in every usable frame (tests/test_compensate_float_cases.py)
    g = _graph(tmp_path, q, floats, w, h, bits, fmt)
    _, path = g.run("compensate", *vc.cli("s", blk[1]), *vc.cli("a", blk[2]), "c.thsad=%d" % thsad, "x.delta=2")
    vc.same(g.read(path), want, name)


@gpu
def test_compensaten_on_a_float_clip_is_the_restatement(oracle, tmp_path):
    case = vc.COMP_N_CASE
    fmt, bits, blk, tr, w, h, thsad = case
    q, floats = vc.comp_clip(case)
    want = vc.compensate_n_expected(oracle, case, q, floats)
    g = _graph(tmp_path, q, floats, w, h, bits, fmt)
    r, path = g.run("multicompensate", *vc.cli("s", blk[1]), "m.radius=%d" % tr, *vc.cli("m", blk[2]), "f.thsad=%d" % thsad)
    assert "multicompensate frames=%d fps=%d/1" % (len(q) * (2 * tr + 1), 24 * (2 * tr + 1)) in r.stdout
    vc.same(g.read(path, len(want)), want, "CompensateN")


@gpu
@pytest.mark.parametrize("name", list(vc.FPS_CASES))
def test_blockfps_on_a_float_clip_is_the_restatement(oracle, tmp_path, name):
    case = vc.FPS_CASES[name]
    fmt, bits, blk, w, h, mode, ml = case
    q, floats = vc.fps_clip(case)
    want, times = vc.fps_expected(oracle, case, q, floats)
    assert 0 in times and any(times)
    g = _graph(tmp_path, q, floats, w, h, bits, fmt)
    r, path = g.run("blockfps", *vc.cli("s", blk[1]), *vc.cli("a", blk[2]), "b.num=60", "b.den=1", "b.mode=%d" % mode, "b.ml=%s" % ml)
    assert "blockfps frames=11 fps=60/1" in r.stdout
    vc.same(g.read(path, 11), want, name)


# ---------------------------------------------------------------------------------------------------- GPU: FlowInter, FlowFPS, Flow, FlowBlur

FLOW_PIPELINE = {"inter": "flowinter", "fps": "flowfps", "flow": "flow", "blur": "flowblur"}


@gpu
@pytest.mark.parametrize("case", vc.FLOWINTER_CASES + vc.FLOWFPS_CASES + vc.FLOW_CASES + vc.BLUR_CASES, ids=lambda c: "%s-%s" % (c.kind, c.name))
def test_the_flow_filters_on_a_float_clip_are_the_restatements(oracle, tmp_path, case):
    c = case
    q, floats, e = vc.flow_expected(oracle, c)
    (vc.flc if c.kind in ("inter", "fps") else vc.fmc).check_conditions(c, e)   # a copying or blending job beside the interpolated ones, taps taken (the modules' own)
    if c.kind == "fps":
        assert 0 in e.times and "copy" in e.kinds                               # an output frame at time256 0: a copy
    g = _graph(tmp_path, q, floats, c.w, c.h, c.bits, c.fmt)
    r, path = g.run(FLOW_PIPELINE[c.kind], *vc.flow_cli(c))
    if c.kind == "fps":
        assert "flowfps frames=%d " % e.num_frames in r.stdout
    vc.same(g.read(path, len(e.frames)), e.frames, c.name)


# ---------------------------------------------------------------------------------------------------- GPU: DepanCompensate, DepanStabilise

def _pan(oracle, tmp_path, shape):
    fmt, w, h = vc.PAN_SHAPES[shape]
    frames = vc.pan_clip(fmt, w, h)
    floats = fc.float_clip(frames, 8, seed=9)
    assert any((p.shape[1] * 4) % 256 for p in floats[0]) == (shape != "420-128x96")   # the rows of the two other shapes do not fill their device pitch
    return fmt, w, h, vc.pan_motions(oracle, frames, fmt, w, h), vc.Graph(tmp_path, frames, floats, w, h, 8, fmt)


DEPAN_RUN = ("x.data=analyse", "x.vectors=fw", "a.blksize=8", "a.overlap=4")
NEAREST, BILINEAR, BICUBIC_MIRROR = dict(offset="1.0", subpixel=0), dict(offset="-1.0", subpixel=1), dict(offset="1.0", subpixel=2, mirror=15, blur=2)


@gpu
@pytest.mark.parametrize("shape,fargs", [("420-128x96", NEAREST), ("420-128x96", BILINEAR), ("420-128x96", BICUBIC_MIRROR), ("444-70x54", BICUBIC_MIRROR), ("422-100x72", BILINEAR)],
                         ids=["420-nearest", "420-bilinear", "420-bicubic-mirror", "444-70x54-bicubic-mirror", "422-100x72-bilinear"])
def test_depancompensate_on_a_float_clip_is_the_restatement(oracle, tmp_path, shape, fargs):
    import test_vs_depan_shell as ds
    fmt, w, h, motions, g = _pan(oracle, tmp_path, shape)
    offset = float(fargs["offset"])
    want, warped, stats = [], 0, {}
    for n in range(vc.PAN_NF):
        fm = dr.frame_map(offset, n, vc.PAN_NF)
        if fm is None:
            want.append(g.floats[n])
            continue
        nsrc, start, end = fm
        trsum, _ = dr.motion_to_transform([motions[k] for k in range(start + 1, end + 1)], offset, w, h)
        warped += not np.array_equal(trsum, dr.null())
        want.append(dfr.compensate_frame(g.floats[nsrc], trsum, fargs["subpixel"], vc.SUB[fmt], False, fargs.get("mirror", 0), fargs.get("blur", 0), stats=stats))
    assert warped >= 4
    mirrored = sum(stats.get(k, 0) for k in ("mtop", "mbottom", "mleft", "mright"))
    assert (mirrored > 0 and stats["border"] == 0) if fargs.get("mirror") else (mirrored == 0 and stats["border"] > 0), stats   # samples beyond the frame: mirrored, or the border value
    r, path = g.run("depancompensate", *DEPAN_RUN, *vc.cli("f", fargs))
    got, _, _ = ds.printed(r.stdout)
    assert [ds._bits(m) for m in got] == [ds._bits(m) for m in motions]
    vc.same(g.read(path), want, "DepanCompensate")


@gpu
@pytest.mark.parametrize("shape", ["420-128x96", "444-70x54"])
def test_depanstabilise_on_a_float_clip_fills_from_both_neighbours(oracle, tmp_path, shape):
    import test_vs_depan_shell as ds
    fmt, w, h, motions, g = _pan(oracle, tmp_path, shape)
    fargs = dict(ds.STAB, method=1)
    e = sr.Stabilise(w, h, vc.PAN_NF, fps=(24, 1), **ds._stab_kw(fargs))
    plans = [e.plan(n, motions) for n in range(vc.PAN_NF)]
    src = lambda s: None if s is None else (g.floats[s["frame"]], s["tr"])
    stats, want = {}, []
    for n, p in enumerate(plans):
        want.append(dfr.paint(g.floats[n], p["tr"], src(p["prev"]), src(p["next"]), fargs["subpixel"], vc.SUB[fmt], False, fargs["mirror"], fargs["blur"], stats))
    assert all(p["prev"] is not None and p["next"] is not None for p in plans) and stats["from_prev"] and stats["from_next"] and stats["from_cur"], stats
    r, path = g.run("depanstabilise", *DEPAN_RUN, *vc.cli("f", fargs))
    got, _, _ = ds.printed(r.stdout)
    assert [ds._bits(m) for m in got] == [ds._bits(m) for m in motions]
    vc.same(g.read(path), want, "DepanStabilise")


@gpu
@pytest.mark.parametrize("switch", ["1", "0"], ids=["float-on", "float-off"])
def test_filters_that_read_no_sample_pass_a_float_clip_through_as_before(oracle, tmp_path, switch):
    """mv.DepanAnalyse and mv.SCDetection copy the frames of `clip` and attach properties; they take a float clip with and without the switch, as the reference does, and
    hand its planes to no kernel: the output frames are the float clip's, bit for bit"""
    assert _refusal("DepanAnalyse", "x.float=clip", MVX_VS_FLOAT=switch) == "OK 70x54 frames=4 sample=float bits=32 ssw=1 ssh=1 planes=3"
    assert _refusal("SCDetection", "x.float=clip", MVX_VS_FLOAT=switch) == "OK 70x54 frames=4 sample=float bits=32 ssw=1 ssh=1 planes=3"
    fmt, w, h, motions, g = _pan(oracle, tmp_path, "444-70x54")
    r, path = g.run("depananalyse", "x.vectors=fw", "a.blksize=8", "a.overlap=4", env={"MVX_VS_FLOAT": switch})
    vc.same(g.read(path), g.floats, "DepanAnalyse returns the float clip's frames")


# ---------------------------------------------------------------------------------------------------- GPU: refusals that need frame 0 of a vector clip

def _refusal(filt, *args, **env):
    r = subprocess.run([shim.HOST, shim.PLUGIN, "error", filt, "70", "54", "16"] + list(args), capture_output=True, text=True, timeout=120, env=shim.proc_env(**dict(vc.ENV, **env)))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


@gpu
@pytest.mark.parametrize("filt,args", [("Compensate", ()), ("BlockFPS", ()), ("DegrainN", ("m.radius=1",)), ("CompensateN", ("m.radius=1",)), ("Flow", ()), ("FlowBlur", ())])
def test_clip_and_super_clip_of_unlike_sample_types_draw_the_librarys_messages(filt, args):
    assert _refusal(filt, "x.float=clip", *args) == "ERROR %s: the float entry needs a float super clip." % filt
    assert _refusal(filt, "x.float=super", *args) == "ERROR %s: float super clips are not supported." % filt
    assert _refusal(filt, "x.float=both", *args).startswith("OK ") and _refusal(filt, "x.float=both", *args).split()[3:5] == ["sample=float", "bits=32"]


@gpu
def test_what_has_no_float_entry_refuses_float_clips_and_float_super_clips():
    assert _refusal("DegrainN", "x.float=both", "m.radius=1", "f.out16=1") == "ERROR DegrainN: out16 is not supported on float clips."
    assert _refusal("Degrain1", "x.float=super") == "ERROR Degrain: float super clips are not supported."
    assert _refusal("Degrain1", "x.float=both") == "ERROR Degrain: float super clips are not supported."
    assert _refusal("Degrain1", "x.float=clip") == "ERROR " + FORMAT_MSG % "Degrain1"
    assert _refusal("Mask", "x.float=clip") == "ERROR Mask: input clip must be GRAY8, YUV420P8, YUV422P8, YUV440P8, or YUV444P8, with constant dimensions."
    for filt in ("Compensate", "Flow"):
        assert _refusal(filt, "x.float=both", "f.fields=1") == "ERROR %s: fields is not supported on float clips." % filt
    assert _refusal("CompensateN", "x.float=both", "m.radius=1", "f.fields=1") == "ERROR CompensateN: fields is not supported."   # (for every clip, integer or float)
    # without the float switch a float clip meets today's messages, whatever the other switches say: mv.Compensate tests the sizes first (MVCompensate.c:535-545: a
    # 32-bit clip is not its 16-bit super clip's source), mv.BlockFPS and mv.DegrainN the format
    assert _refusal("Compensate", "x.float=clip", MVX_VS_FLOAT="0") == "ERROR Compensate: wrong source or super clip frame size."
    assert _refusal("BlockFPS", "x.float=clip", MVX_VS_FLOAT="0") == "ERROR " + FORMAT_MSG % "BlockFPS"
    assert _refusal("DegrainN", "x.float=clip", "m.radius=1", MVX_VS_FLOAT="0") == "ERROR " + FORMAT_MSG % "DegrainN"
