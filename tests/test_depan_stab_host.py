"""CPU tests of mv.DepanStabilise's host side: creation (no device is touched) against the restatement tests/depan_stab_ref.py, with the reference's
messages in its order (MVDepan.cpp:3975-4055) and the library's own refusals; the derived constants and the window tables; the struct layouts
against the C header; and the plans (csrc/mvx_depan_stab_host.h through mvx_depan_stabilise_plan) bit for bit against the restatement over
whole synthetic motion tracks.  Every comparison is exact: floats by their bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depan_stab_cases as sc
import depan_stab_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W, H = 206, 118


def _bits(v):
    return np.asarray(v, dtype=f32).view(np.uint32).tolist()


def pair(mv, n, w=W, h=H, fps=(25, 1), fmt=None, **kw):
    fmt = fmt or {}
    return mv.DepanStabilise(w, h, num_frames=n, fps=fps, **fmt, **kw), sr.Stabilise(w, h, n, fps=fps, **fmt, **kw)


# ------------------------------------------------------------------------------------------------ creation

BAD = [dict(cutoff=0.0), dict(cutoff=-1.0), dict(prev=-1), dict(next=-2), dict(subpixel=3), dict(subpixel=-1), dict(pixaspect=0.0), dict(mirror=16), dict(mirror=-1),
       dict(blur=-1), dict(method=2), dict(method=-1), dict(bits=17), dict(subsampling=(0, 1)), dict(subsampling=(2, 1)), dict(fps=(0, 1)), dict(fps=(25, 0)),
       dict(data_frames=9)]
_ORDER = dict(cutoff=0.0, prev=-1, next=-1, subpixel=5, pixaspect=-1.0, mirror=99, blur=-3, method=7, bits=32, fps=(0, 0), data_frames=1)
BAD += [dict(list(_ORDER.items())[k:]) for k in range(len(_ORDER))]          # several wrong at once: the earliest in the reference's order wins
TEXTS = ["cutoff must be greater than 0.", "prev must not be negative.", "next must not be negative.", "subpixel must be between 0 and 2 (inclusive).",
         "pixaspect must be greater than 0.", "mirror must be between 0 and 15 (inclusive).", "blur must not be negative.", "method must be between 0 and 1 (inclusive).",
         "clip must have constant format and dimensions, integer sample type, bit depth up to 16, and it must be Gray, 420, 422, or 444, and not RGB.",
         "clip must have known frame rate.", "data must have at least as many frames as clip."]


def _create(mv, kw, cls):
    kw = dict(kw)
    fps, bits, sub, df = kw.pop("fps", (25, 1)), kw.pop("bits", 8), kw.pop("subsampling", (1, 1)), kw.pop("data_frames", None)
    if cls == "lib":
        return mv.DepanStabilise(W, H, bits, sub, num_frames=10, fps=fps, data_frames=df, **kw)
    return sr.Stabilise(W, H, 10, fps=fps, bits=bits, subsampling=sub, data_frames=df, **kw)


@pytest.mark.parametrize("kw", BAD, ids=repr)
def test_creation_fails_with_the_reference_s_message(mv, kw):
    with pytest.raises(ValueError) as want:
        _create(mv, kw, "ref")
    with pytest.raises(mv.MvtoolsError) as got:
        _create(mv, kw, "lib")
    assert str(got.value) == str(want.value)


def test_the_messages_in_the_reference_s_order(mv):
    for k in range(len(_ORDER)):
        with pytest.raises(mv.MvtoolsError) as got:
            _create(mv, dict(list(_ORDER.items())[k:]), "lib")
        assert str(got.value) == "DepanStabilise: " + TEXTS[k]


def test_the_library_s_own_refusals(mv):
    size = "DepanStabilise: every plane must be at least 2 samples wide and 2 high, and the frame at most 32767 x 32767."
    pitch = "DepanStabilise: pitches must hold a row of their plane and be multiples of the sample size."
    rate = "DepanStabilise: the frame rate must be positive, and fps / (4 * cutoff) below 1048576."
    for args, kw, text in (((3, 64), {}, size), ((64, 3), {}, size), ((1, 64), dict(gray=True), size), ((32768, 64), {}, size),
                           ((64, 64), dict(src_pitch=[63, 32, 32]), pitch), ((64, 64), dict(bits=16, dst_pitch=[129, 64, 64]), pitch),
                           ((64, 64), dict(dst_pitch=[64, 31, 32]), pitch), ((64, 64), dict(num_frames=0), "DepanStabilise: clip must have at least one frame."),
                           ((64, 64), dict(fps=(-25, 1)), rate), ((64, 64), dict(cutoff=1e-6), rate), ((64, 64), dict(cutoff=float("nan")), rate),
                           ((64, 64), dict(tzoom=-1.0), "DepanStabilise: tzoom must not be negative."), ((64, 64), dict(tzoom=float("nan")), "DepanStabilise: tzoom must not be negative.")):
        with pytest.raises(mv.MvtoolsError) as got:
            mv.DepanStabilise(*args, **dict(dict(num_frames=10), **kw))
        assert str(got.value) == text, (args, kw)
    # the reference's messages come first
    with pytest.raises(mv.MvtoolsError) as got:
        mv.DepanStabilise(3, 64, num_frames=10, method=2, tzoom=-1.0)
    assert str(got.value) == "DepanStabilise: method must be between 0 and 1 (inclusive)."
    mv.DepanStabilise(2, 2, gray=True, num_frames=1)
    mv.DepanStabilise(4, 4, num_frames=1, tzoom=0.0)


GOOD = [dict(), dict(cutoff=0.5), dict(cutoff=2.0), dict(cutoff=7.0), dict(cutoff=0.5, tzoom=0.5), dict(cutoff=0.5, tzoom=0.0), dict(fps=(30000, 1001), damping=0.5),
        dict(initzoom=1.1, zoommax=1.05), dict(initzoom=1.1, zoommax=-1.05), dict(zoommax=1.0), dict(zoommax=-1.0), dict(dxmax=0.0, dymax=0.0, rotmax=0.0),
        dict(dxmax=-40.0, dymax=-20.0, rotmax=-2.0, zoommax=-1.2), dict(fields=1, pixaspect=1.0940), dict(fps=(5, 1), cutoff=2.0),
        dict(bits=10, subsampling=(1, 0), blur=5), dict(bits=16, subsampling=(0, 0), blur=5), dict(bits=12, gray=True, blur=3), dict(blur=7, mirror=15, subpixel=0)]


@pytest.mark.parametrize("kw", GOOD, ids=repr)
def test_derived_constants_equal_the_restatement_s(mv, kw):
    kw = dict(kw)
    fmt = {k: kw.pop(k) for k in ("bits", "subsampling", "gray") if k in kw}
    g, e = pair(mv, 50, fps=kw.pop("fps", (25, 1)), fmt=fmt, **kw)
    i = g.info
    assert (i.radius, i.wint_size, i.winrz_size, i.winfz_size, i.nfields, i.pixel_max) == (e.radius, e.wintsize, e.winrzsize, e.winfzsize, e.nfields, e.pixel_max)
    assert _bits([i.fps, i.freqnative, i.initzoom, i.zoommax, i.xcenter, i.ycenter]) == _bits([e.fps, e.freqnative, e.initzoom, e.zoommax, e.xcenter, e.ycenter])
    assert _bits(list(i.nonlinfactor)) == _bits([e.nonlinfactor[k] for k in ("dxc", "dxx", "dxy", "dyc", "dyx", "dyy")])
    for got, want in zip(g.windows(), (e.wint, e.winrz, e.winfz)):
        assert got.shape == (e.radius + 1,) and _bits(got) == _bits(want)
    np_ = 1 if fmt.get("gray") else 3
    sw = 0 if fmt.get("gray") else fmt.get("subsampling", (1, 1))[0]
    half = 1 << (fmt.get("bits", 8) - 1)
    blur = kw.get("blur", 0)
    assert i.num_planes == np_ and list(i.border) == [0, half, half] and list(i.blur) == [blur, blur // 2 if sw else blur, blur // 2 if sw else blur]
    assert (i.subpixel, i.mirror, i.method, i.prev, i.next) == (e.subpixel, e.mirror, e.method, e.prev, e.next)


def test_the_radius_of_the_window_tables(mv):
    """fps 25 / 1: cutoff 0.5, 2.0 and 7.0 give radius 12, 3 and 0; the tables end in a zero, and with radius 0 they are that zero alone"""
    for cutoff, radius in ((0.5, 12), (2.0, 3), (7.0, 0)):
        g, e = pair(mv, 50, cutoff=cutoff)
        assert g.info.radius == e.radius == radius
        wint, winrz, winfz = g.windows()
        assert wint[-1] == 0 and (radius == 0 or wint[0] == 1) and len(wint) == radius + 1


def test_struct_layouts_match_the_header(mv, tmp_path):
    names = ["mvx_depan_stabilise_args", "mvx_depan_stabilise_info", "mvx_depan_stabilise_source", "mvx_depan_stabilise_frame_plan", "mvx_depan_stabilise_job"]
    py = [mv.DepanStabiliseArgs, mv.DepanStabiliseInfo, mv.DepanStabiliseSource, mv.DepanStabilisePlan, mv.DepanStabiliseJob]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvtools_amd.h"', 'int main(void) {']
    for n, t in zip(names, py):
        lines.append('printf("%%zu", sizeof(%s));' % n)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (n, f[0]) for f in t._fields_]
        lines.append('printf("\\n");')
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0;", "}"]))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe])
    for line, t in zip(subprocess.check_output([exe]).decode().split("\n"), py):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, f[0]).offset for f in t._fields_], t.__name__


# ------------------------------------------------------------------------------------------------ plans

def words(plan):
    return np.frombuffer(bytes(plan), dtype=np.uint32).tolist()


def same_plans(g, e, motions, frames=None, stats=None):
    """every frame's window and plan, all 28 words; returns the restatement's plans"""
    out = {}
    for n in (range(e.num_frames) if frames is None else frames):
        w = g.window(n)
        assert w == e.window(n), n
        want = e.plan(n, motions, stats)
        assert words(g.plan(n, motions[w[0]:w[1] + 1])) == sr.plan_words(want), (n, want)
        out[n] = want
    return out


@pytest.mark.parametrize("addzoom", [0, 1])
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("seed", [1, 2])
def test_whole_tracks(mv, method, addzoom, seed):
    """40 frames, every ndest including 0, 1 and the last; a bad frame in the middle moves the base and cuts method 1's window, which turns symmetric"""
    n = 40
    motions = sc.track(n, seed, bad=(17,))
    g, e = pair(mv, n, method=method, addzoom=addzoom, prev=2, next=3, cutoff=0.5)
    st = {}
    plans = same_plans(g, e, motions, stats=st)
    assert plans[17]["base"] and plans[17]["nbase"] == 17 and plans[0]["base"]
    if method == 0:
        assert plans[30]["nbase"] == 17 and plans[16]["nbase"] == 0 and st["scene_start"] == 2
    else:
        assert e.radius == 12 and st["window_cut"] > 0
        assert plans[20]["nbase"] == 17 and plans[14]["nbase"] == 12          # 14: the bad frame 17 cuts nmax to 16, and the base follows to 12
        assert plans[35]["nbase"] == 31                                      # the clip's end cuts too
    assert st["next_cut"] > 0 and st["next_is_current"] > 0                  # frame 16: the frame after it is bad, next names frame 16 itself
    assert plans[16]["next"]["frame"] == 16 and plans[16]["next"]["tr"].tobytes() == plans[16]["tr"].tobytes()
    assert plans[18]["prev"]["frame"] == 17 and plans[19]["prev"]["frame"] == 17 and plans[25]["prev"]["frame"] == 23


def test_prev_larger_than_the_distance_to_the_base_and_the_dead_choice_of_fill_prev(mv):
    """fillBorderPrev assigns nprevbest = n in every iteration (:3412): the source is frame nprev whatever its test of :3415 finds.  The track pans
    steadily, so the restatement's own minimum is at the frame nearest to ndest, not at nprev"""
    n = 20
    motions = [(f32(2.5), f32(-1.5), f32(1), f32(0))] * n
    motions[6] = (f32(0), f32(0), f32(1), f32(0))
    for method in (0, 1):
        g, e = pair(mv, n, method=method, prev=5, cutoff=0.5)
        st = {}
        plans = same_plans(g, e, motions, stats=st)
        assert st["prev_not_centred"] > 0
        k = next(k for k in plans if plans[k]["prev"]["centred"] != plans[k]["prev"]["frame"])
        assert plans[k]["prev"]["frame"] == max(plans[k]["nbase"], k - 5)
        assert plans[15]["prev"]["frame"] == max(plans[15]["nbase"], 10)
        assert plans[8]["prev"]["frame"] == plans[8]["nbase"] and plans[8]["nbase"] in (6, 7)   # prev = 5 reaches past the base


def test_fitlast_reaches_the_clip_s_end(mv):
    n = 30
    motions = sc.track(n, 3)
    g, e = pair(mv, n, fitlast=8, cutoff=0.5, next=1)
    st = {}
    plans = same_plans(g, e, motions, stats=st)
    assert st["fitlast"] == 8                                                # frames 22 .. 29
    assert _bits(plans[29]["motion"][:2]) == _bits([0, 0]) or plans[29]["motion"][0] == 0   # the factor is 0 at the last frame


LIMITS = [(dict(dxmax=0.5), "soft_dx"), (dict(dymax=0.5), "soft_dy"), (dict(rotmax=0.01), "soft_rot"), (dict(zoommax=1.0005, addzoom=1), "soft_zoom"),
          (dict(dxmax=-0.5), "reset_dx"), (dict(dymax=-0.5), "reset_dy"), (dict(rotmax=-0.01), "reset_rot"), (dict(zoommax=-1.0005, addzoom=1), "reset_zoom")]


@pytest.mark.parametrize("kw,counter", LIMITS, ids=[c for _, c in LIMITS])
def test_each_limit_soft_and_resetting(mv, kw, counter):
    n = 30
    motions = sc.track(n, 4, zoom=0.01)
    big = dict(dxmax=1e4, dymax=1e4, rotmax=1e4, zoommax=1e4)
    g, e = pair(mv, n, cutoff=0.5, prev=1, **dict(big, **kw))
    st = {}
    plans = same_plans(g, e, motions, stats=st)
    assert st.get(counter, 0) > 0, st
    if counter.startswith("reset"):
        resets = sum(v for k, v in st.items() if k.startswith("reset_"))        # (a run-away recursion resets through the non-finite test of dx)
        assert sum(1 for p in plans.values() if p["base"]) == resets + 1        # frame 0, and InertialLimit moved the base to ndest


def test_a_non_finite_motion(mv):
    n = 20
    motions = sc.track(n, 5)
    motions[9] = (f32(np.inf), motions[9][1], motions[9][2], motions[9][3])
    motions[14] = (motions[14][0], f32(np.nan), motions[14][2], motions[14][3])
    for method in (0, 1):
        g, e = pair(mv, n, method=method, cutoff=0.5, prev=1, next=1)
        st = {}
        plans = same_plans(g, e, motions, stats=st)
        if method == 0:
            assert st["reset_dx"] > 0 and plans[9]["base"]
        else:
            assert np.isnan(plans[14]["tr"]).any()


def test_radius_zero_gives_nan_bit_for_bit(mv):
    """method 1 with fps < 4 * cutoff: Average divides 0 by 0 (MVDepan.cpp:3155).  Every coefficient arrives as NaN -- the one NaN a plan
    carries (mvtools_amd.h, DepanStabilise divergence 6), compared by its bits like every other value"""
    n = 12
    motions = sc.track(n, 6)
    g, e = pair(mv, n, method=1, cutoff=7.0, prev=1, next=1)
    assert e.radius == 0
    plans = same_plans(g, e, motions)
    assert all(np.isnan(p["tr"]).all() for p in plans.values())
    assert all(np.isnan(g.plan(k, motions[g.window(k)[0]:g.window(k)[1] + 1]).tr[0]) for k in range(n))


def test_fields(mv):
    n = 24
    motions = sc.track(n, 8, bad=(10,))
    for method in (0, 1):
        g, e = pair(mv, n, method=method, fields=1, pixaspect=1.094, cutoff=0.5, prev=2, next=2, addzoom=1)
        assert g.info.nfields == 2
        same_plans(g, e, motions)


def test_a_method_0_base_that_is_not_frame_0(mv):
    """fps 5 / 1, cutoff 2.0: the window reaches 25 frames back.  With the default damping the recursion runs away at this rate within the 25
    frames and InertialLimit's non-finite test moves the base to ndest; with damping 0.2 it does not, and the base stays 25 frames back"""
    n = 40
    motions = sc.track(n, 9)
    g, e = pair(mv, n, fps=(5, 1), cutoff=2.0, prev=3)
    assert g.window(30)[0] == 5 and g.window(25)[0] == 0 and g.window(26)[0] == 1
    st = {}
    plans = same_plans(g, e, motions, stats=st)
    assert plans[30]["base"] and st["reset_dx"] > 0
    g, e = pair(mv, n, fps=(5, 1), cutoff=2.0, prev=3, damping=0.2)
    plans = same_plans(g, e, motions)
    assert plans[30]["nbase"] == 5 and plans[39]["nbase"] == 14 and plans[30]["prev"]["frame"] == 27


def test_the_motions_must_cover_the_window(mv):
    g = mv.DepanStabilise(W, H, num_frames=10, next=2)
    with pytest.raises(mv.MvtoolsError):
        g.plan(4, sc.track(3, 1))
    with pytest.raises(mv.MvtoolsError):
        g.window(10)
