"""CPU tests of the float FlowInter / FlowFPS entries (mvx_flowinter_create_float, mvx_flowfps_create_float; no create touches a device and
mvx_flow_frames checks its jobs before any launch): every creation message in its order with the float-specific one after the frame-size
checks and the library's geometry and pitch checks last, the integer creates' unchanged refusal of a float super clip and their own order,
pitches and job layouts at a sample size of 4, get_info / map against the integer objects', the package's sample_float keyword -- and
csrc/mvx_flow_float_rule.h as a stand-alone host program (with AddressSanitizer and UBSan where g++ links them) against
tests/flow_float_ref.py, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import flow_float_ref as fl
from test_block_host import _clips, _copy, _err, _split_uv_pitch
from test_float_host import CSRC, HERE, _sanitizer_flags

ROWS = [320 * 4, 160 * 4, 160 * 4]   # rows of 320 / 160 float samples
FPITCH = [1280, 768, 768]            # ... rounded up to 256 bytes
IPITCH = [320, 160, 160]


def _fsup(mv, w=320, h=192, **kw):
    return mv.Super(w, h, 32, sample_float=True, **kw)


def _inter(mv, sup, bw, fw, pitch=FPITCH, **kw):
    return mv.FlowInter(sup, bw, fw, 10, pitch, sample_float=True, **kw)


def _fps(mv, sup, bw, fw, fps=(24, 1), pitch=FPITCH, **kw):
    return mv.FlowFPS(sup, bw, fw, 10, pitch, fps[0], fps[1], sample_float=True, **kw)


def test_flowinter_float_messages_and_their_order(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    needs, size = "FlowInter: the float entry needs a float super clip.", "FlowInter: wrong source or super clip frame size."
    time = "FlowInter: time must be between 0 and 100 % (inclusive)."
    assert _err(lambda: _inter(mv, fsup, bw, fw, time=-0.5)) == time
    assert _err(lambda: _inter(mv, isup, bw, fw, time=100.5, ml=0.0)) == time           # (before the kind of super clip)
    assert _err(lambda: _inter(mv, fsup, bw, fw, ml=0.0, thscd1=16321)) == "FlowInter: ml must be greater than 0."
    assert _err(lambda: _inter(mv, fsup, bw, fw, thscd1=16321)) == "FlowInter: thscd1 can be at most 16320."
    _inter(mv, fsup, bw, fw, thscd1=16320, time=0.0)
    _inter(mv, fsup, bw, fw, time=100.0, blend=0)
    # the similarity check: the LAST mismatching field's message wins
    assert _err(lambda: _inter(mv, fsup, bw, _copy(mv, fw, nWidth=336))) == "FlowInter: mvbw and mvfw have different widths."
    assert _err(lambda: _inter(mv, isup, bw, _copy(mv, fw, nWidth=336, nPel=4))) == "FlowInter: mvbw and mvfw have different pel precision."
    assert _err(lambda: _inter(mv, fsup, bw, _copy(mv, fw, nHeight=200, bitsPerSample=16))) == "FlowInter: mvbw and mvfw have different bit depths."
    assert _err(lambda: _inter(mv, fsup, _copy(mv, bw, nDeltaFrame=0), _copy(mv, fw, nDeltaFrame=0))) == \
        "FlowInter: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _inter(mv, fsup, bw, _copy(mv, fw, nDeltaFrame=2))) == "FlowInter: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _inter(mv, fsup, fw, fw)) == "FlowInter: mvbw must be generated with isb=True."
    assert _err(lambda: _inter(mv, isup, bw, bw)) == "FlowInter: mvfw must be generated with isb=False."
    assert _err(lambda: _inter(mv, _fsup(mv, w=336), bw, fw)) == size
    assert _err(lambda: _inter(mv, _fsup(mv, pel=4), bw, fw)) == size
    assert _err(lambda: _inter(mv, _fsup(mv, w=336), bw, bw)) == "FlowInter: mvfw must be generated with isb=False."
    # an integer super clip handed to the float entry: after the frame size, before the geometry and the pitches
    assert _err(lambda: _inter(mv, isup, bw, fw)) == needs
    assert _err(lambda: _inter(mv, isup, bw, fw, pitch=[4, 4, 4])) == needs
    assert _err(lambda: _inter(mv, mv.Super(336, 192, 8), bw, fw)) == size
    sup16, bw16, fw16 = _clips(mv, bits=16)
    assert _err(lambda: _inter(mv, sup16, bw16, fw16)) == needs
    _inter(mv, fsup, bw16, fw16)                                                        # vectors of a 16-bit search
    # the library's own checks come last: the frame size is said before a pitch, where the integer entry says the pitch first
    assert _err(lambda: _inter(mv, _fsup(mv, w=336), bw, fw, pitch=[4, 4, 4])) == size
    assert _err(lambda: mv.FlowInter(mv.Super(336, 192, 8), bw, fw, 10, [4, 4, 4])).startswith("FlowInter: clip pitch of plane 0 must hold a row of 320 bytes")
    tiny = _fsup(mv, w=8, h=64)
    isup8 = mv.Super(8, 64, 8)
    tb, tf = mv.Analyse(isup8, isb=1, blksize=8, overlap=0).ad, mv.Analyse(isup8, isb=0, blksize=8, overlap=0).ad
    two = "FlowInter: the frame must be at least two blocks wide and two blocks high."
    assert _err(lambda: mv.FlowInter(tiny, tb, tf, 10, [32, 16, 16], sample_float=True)) == two
    assert _err(lambda: mv.FlowInter(isup8, tb, tf, 10, [32, 16, 16], sample_float=True)) == needs
    assert _err(lambda: _inter(mv, _split_uv_pitch(_fsup(mv)), bw, fw)) == "FlowInter: U and V super planes must share one pitch."
    assert _err(lambda: _inter(mv, _split_uv_pitch(_fsup(mv)), bw, fw, time=101.0)) == time
    # the integer entry keeps its refusal, first of all
    assert _err(lambda: mv.FlowInter(fsup, bw, fw, 10, FPITCH, time=500.0, ml=-1.0)) == "FlowInter: float super clips are not supported."


def test_flowfps_float_messages_and_their_order(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    needs, size = "FlowFPS: the float entry needs a float super clip.", "FlowFPS: wrong source or super clip frame size."
    rate = "FlowFPS: The input clip must have a frame rate. Invoke AssumeFPS if necessary."
    source = "FlowFPS: inconsistent source and vector frame size."
    clips = "FlowFPS: inconsistent clips frame size! Incomprehensible error messages are the best, right?"
    assert _err(lambda: _fps(mv, fsup, bw, fw, mask=3)) == "FlowFPS: mask must be 0, 1, or 2."
    assert _err(lambda: _fps(mv, isup, bw, fw, mask=-1, ml=-1.0)) == "FlowFPS: mask must be 0, 1, or 2."
    assert _err(lambda: _fps(mv, fsup, bw, fw, ml=0.0, thscd1=20000)) == "FlowFPS: ml must be greater than 0."
    assert _err(lambda: _fps(mv, fsup, bw, fw, thscd1=20000)) == "FlowFPS: thscd1 can be at most 16320."
    assert _err(lambda: _fps(mv, fsup, bw, _copy(mv, fw, nBlkSizeX=16, nOverlapY=2))) == "FlowFPS: mvbw and mvfw have different overlap."
    assert _err(lambda: _fps(mv, fsup, _copy(mv, bw, nDeltaFrame=-1), _copy(mv, fw, nDeltaFrame=-1))) == \
        "FlowFPS: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _fps(mv, fsup, bw, _copy(mv, fw, nDeltaFrame=3))) == "FlowFPS: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _fps(mv, isup, fw, fw)) == "FlowFPS: mvbw must be generated with isb=True."
    assert _err(lambda: _fps(mv, fsup, bw, bw, fps=(0, 1))) == "FlowFPS: mvfw must be generated with isb=False."
    assert _err(lambda: _fps(mv, fsup, bw, fw, fps=(0, 1))) == rate
    assert _err(lambda: _fps(mv, _fsup(mv, w=336), bw, fw, fps=(24, 0))) == rate
    assert _err(lambda: _fps(mv, _fsup(mv, w=336), bw, fw)) == source
    assert _err(lambda: _fps(mv, _fsup(mv, pel=1), bw, fw)) == size
    assert _err(lambda: _fps(mv, fsup, _copy(mv, bw, nHPadding=8), fw)) == clips
    # an integer super clip handed to the float entry: after all of these, before the geometry and the pitches
    assert _err(lambda: _fps(mv, isup, bw, fw)) == needs
    assert _err(lambda: _fps(mv, isup, bw, fw, pitch=[4, 4, 4])) == needs
    assert _err(lambda: _fps(mv, isup, _copy(mv, bw, nHPadding=8), fw)) == clips
    assert _err(lambda: _fps(mv, mv.Super(336, 192, 8), bw, fw)) == source
    sup16, bw16, fw16 = _clips(mv, bits=16)
    assert _err(lambda: _fps(mv, sup16, bw16, fw16)) == needs
    _fps(mv, fsup, bw16, fw16, num=60, den=1, mask=1, blend=0)
    # the library's own checks come last, where the integer entry says them before the rate and the frame sizes
    assert _err(lambda: _fps(mv, fsup, bw, fw, fps=(0, 1), pitch=[4, 4, 4])) == rate
    assert _err(lambda: mv.FlowFPS(isup, bw, fw, 10, [4, 4, 4], 0, 1)).startswith("FlowFPS: clip pitch of plane 0 must hold a row of 320 bytes")
    assert _err(lambda: _fps(mv, _split_uv_pitch(_fsup(mv)), bw, fw)) == "FlowFPS: U and V super planes must share one pitch."
    assert _err(lambda: _fps(mv, _split_uv_pitch(_fsup(mv)), bw, fw, fps=(0, 1))) == rate
    assert _err(lambda: mv.FlowFPS(fsup, bw, fw, 10, FPITCH, 0, 1, mask=9)) == "FlowFPS: float super clips are not supported."


def test_pitches_of_the_float_entries(mv):
    """clip and dst: any pitch that holds a row and is a multiple of 4; super: multiples of 16"""
    _, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    msg = lambda name, what, p: "%s: %s pitch of plane %d must hold a row of %d bytes and be a multiple of the sample size." % (name, what, p, ROWS[p])
    for name, make in (("FlowInter", lambda **kw: _inter(mv, fsup, bw, fw, **kw)), ("FlowFPS", lambda **kw: _fps(mv, fsup, bw, fw, **kw))):
        assert make().dst_pitch == FPITCH
        make(pitch=ROWS)
        make(pitch=[ROWS[0] + 4, ROWS[1], ROWS[2] + 256])                # an odd number of samples; U and V differ
        assert make(pitch=ROWS, dst_pitch=[ROWS[0] + 12, ROWS[1] + 4, ROWS[2]]).dst_pitch == [ROWS[0] + 12, ROWS[1] + 4, ROWS[2]]
        assert _err(lambda: make(pitch=[ROWS[0] + 2, ROWS[1], ROWS[2]])) == msg(name, "clip", 0)
        assert _err(lambda: make(pitch=[ROWS[0], ROWS[1] - 4, ROWS[2]])) == msg(name, "clip", 1)
        assert _err(lambda: make(pitch=[ROWS[0], ROWS[1], ROWS[2] + 1])) == msg(name, "clip", 2)
        assert _err(lambda: make(pitch=ROWS, dst_pitch=[ROWS[0], ROWS[1] + 2, ROWS[2]])) == msg(name, "dst", 1)
        assert _err(lambda: make(pitch=ROWS, dst_pitch=[ROWS[0] - 4, ROWS[1], ROWS[2]])) == msg(name, "dst", 0)
        assert _err(lambda: make(pitch=IPITCH)) == msg(name, "clip", 0)  # the integer clip's pitches
    odd = _fsup(mv)
    odd.pitch = [odd.pitch[0] + 8, odd.pitch[1], odd.pitch[2]]
    assert _err(lambda: _inter(mv, odd, bw, fw)).startswith("FlowInter: super pitch of plane 0 must hold a row of ")
    assert _err(lambda: _fps(mv, odd, bw, fw)).startswith("FlowFPS: super pitch of plane 0 must hold a row of ")


@pytest.mark.parametrize("rate", [dict(num=60, den=1), dict(num=48, den=1), dict(), dict(num=0, den=0), dict(num=30000, den=1001)], ids=["60", "48", "25", "double", "ntsc"])
@pytest.mark.parametrize("delta", [1, 2])
def test_flowfps_info_and_map_are_the_integer_objects(mv, rate, delta):
    isup, bw, fw = _clips(mv, delta=delta)
    new, old = _fps(mv, _fsup(mv), bw, fw, **rate), mv.FlowFPS(isup, bw, fw, 10, IPITCH, 24, 1, **rate)
    assert (new.num_frames, new.fps_num, new.fps_den) == (old.num_frames, old.fps_num, old.fps_den)
    assert [new.map(n) for n in range(new.num_frames + 2)] == [old.map(n) for n in range(old.num_frames + 2)]
    if rate == dict(num=60, den=1) and delta == 1:
        assert new.num_frames == 23 and [new.map(n)[2] for n in range(6)] == [0, 102, 205, 51, 154, 0]
    if rate == dict(num=48, den=1) and delta == 1:
        assert [new.map(n) for n in range(3)] == [(0, 1, 0), (0, 1, 128), (1, 2, 0)]


def test_flowinter_map_is_the_integer_objects(mv):
    isup, bw, fw = _clips(mv, delta=2)
    for time, want in [(0.39062499, 1), (50.0, 128), (0.0, 0), (100.0, 256), (37.5, 96), (99.9, 255)]:
        new, old = _inter(mv, _fsup(mv), bw, fw, time=time), mv.FlowInter(isup, bw, fw, 10, IPITCH, time=time)
        assert new.map(5) == old.map(5) == (5, 7, want)
        assert (new.num_frames, new.fps_num, new.fps_den) == (old.num_frames, old.fps_num, old.fps_den) == (10, 0, 0)


def test_flow_frames_checks_its_jobs_before_any_device_call(mv):
    _, bw, fw = _clips(mv)
    L, A = mv.lib(), 0x10000  # never dereferenced
    job = (mv.FlowJob * 2)()

    def checks(g, fps):
        def fill(left=(A, A, A), right=(A, A, A), dst=(A, A, A), supl=(A, A, A), supr=(A, A, A), t=128, k=0):
            for j in range(2):
                job[j].time256 = 128
                for p in range(3):
                    job[j].clip_left[p], job[j].clip_right[p], job[j].dst[p], job[j].super_left[p], job[j].super_right[p] = A, A, A, A, A
            job[k].time256 = t
            for p in range(3):
                job[k].clip_left[p], job[k].clip_right[p], job[k].dst[p], job[k].super_left[p], job[k].super_right[p] = left[p], right[p], dst[p], supl[p], supr[p]
            assert L.mvx_flow_frames(g.h, 2, job, None) == -1
            return L.mvx_last_error().decode()
        assert fill(t=257) == "mvx_flow_frames: time256 must be between 0 and 256"
        assert fill(left=(None, A, A)) == "mvx_flow_frames: dst / clip_left / clip_right are required"
        assert fill(dst=(None, A, A), k=1) == "mvx_flow_frames: dst / clip_left / clip_right are required"
        assert fill(left=(A + 2, A, A)) == "mvx_flow_frames: clip_left plane 0 must be aligned to 4 bytes"
        assert fill(left=(A, A, None)) == "mvx_flow_frames: clip_left plane 2 is required"
        assert fill(right=(A, A + 6, A), k=1) == "mvx_flow_frames: clip_right plane 1 must be aligned to 4 bytes"
        assert fill(dst=(A, A, A + 1)) == "mvx_flow_frames: dst plane 2 must be aligned to 4 bytes"
        assert fill(dst=(A, None, A), k=1) == "mvx_flow_frames: dst plane 1 is required"
        assert fill(supl=(A + 4, A, A)) == "mvx_flow_frames: super_left plane 0 must be aligned to 16 bytes"
        assert fill(supr=(A, A + 8, A), k=1) == "mvx_flow_frames: super_right plane 1 must be aligned to 16 bytes"
        if fps:   # a copy of the left frame still needs it aligned; the right frame is not looked at
            assert fill(left=(A + 2, A, A), t=0) == "mvx_flow_frames: clip_left plane 0 must be aligned to 4 bytes"
            assert fill(right=(A, A + 2, A), t=256) == "mvx_flow_frames: clip_right plane 1 must be aligned to 4 bytes"
        assert L.mvx_flow_frames(g.h, 0, job, None) == 0
    checks(_inter(mv, _fsup(mv), bw, fw), False)
    checks(_fps(mv, _fsup(mv), bw, fw), True)


def test_the_keyword_selects_the_float_entries_and_nothing_else_changes(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    pairs = ((lambda s: _inter(mv, s, bw, fw), lambda s: mv.FlowInter(s, bw, fw, 10, IPITCH)),
             (lambda s: _fps(mv, s, bw, fw), lambda s: mv.FlowFPS(s, bw, fw, 10, IPITCH, 24, 1)))
    for make, plain in pairs:
        new, old = make(fsup), plain(isup)
        assert new.is_float and not old.is_float
        assert new.dst_pitch == FPITCH and old.dst_pitch == IPITCH
        assert _err(lambda: plain(fsup)).endswith("float super clips are not supported.")
        assert _err(lambda: make(isup)).endswith("the float entry needs a float super clip.")
    assert np.dtype(fsup.dtype) == np.float32
    L = mv.lib()
    assert L.mvx_flowinter_create_float.argtypes == L.mvx_flowinter_create.argtypes and L.mvx_flowfps_create_float.argtypes == L.mvx_flowfps_create.argtypes


# ------------------------------------------------------------------------------------------------ the rule header on the host

@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    assert shutil.which("g++"), "the host program needs g++"
    tmp = str(tmp_path_factory.mktemp("flow_float_rule"))
    exe = os.path.join(tmp, "flow_float_rule_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + CSRC, os.path.join(HERE, "flow_float_rule_host_main.cpp"),
                           "-o", exe] + _sanitizer_flags(tmp))
    return exe


MASKS = (0, 1, 127, 128, 254, 255)


def test_rule_header_on_the_host_is_the_restatement(rule_exe):
    """every time256 0..256 against every pair of masks at 0 / 1 / 127 / 128 / 254 / 255, random samples -- luma-like, chroma-like (negative)
    and overshooting, a few equal and a few zeros of either sign for the minimum and maximum -- bit for bit tests/flow_float_ref.py"""
    rng = np.random.default_rng(811)
    t, mF, mB, _ = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(0, 257), MASKS, MASKS, np.arange(12), indexing="ij"))
    n = t.size
    f = (rng.random((6, n)) * 1.5 - 0.2).astype(np.float32)
    f[:, ::3] -= np.float32(0.5)
    f[1, ::7] = f[0, ::7]                                     # dB == dF
    f[4, ::11], f[5, ::13] = f[0, ::11], f[1, ::13]           # an extra fetch on a bound of the clamp
    f[0, ::17], f[1, ::17] = np.float32(0.0), np.float32(-0.0)
    f[1, 5::34], f[0, 5::34] = np.float32(0.0), np.float32(-0.0)
    k = np.stack([mF, mB, t]).astype(np.int32)
    r = subprocess.run([rule_exe, str(n)], input=f.tobytes() + k.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    out = np.frombuffer(r.stdout, np.float32).reshape(4, n)
    dF, dB, dF0, dB0, dFF, dBB = f
    MF, MB = mF.astype(np.int64), mB.astype(np.int64)
    for tt in range(257):
        s = t == tt
        a = (dF[s], dB[s])
        want = (fl.simple(tt, *a, MF[s], MB[s]), fl.regular(tt, *a, dF0[s], dB0[s], MF[s], MB[s]), fl.extra(tt, *a, dFF[s], dBB[s], MF[s], MB[s]),
                fl.blend(tt, dF0[s], dB0[s]))
        for i, (w, what) in enumerate(zip(want, ("simple", "regular", "extra", "blend"))):
            assert w.dtype == np.float32 and np.array_equal(fl.bits(out[i][s]), fl.bits(w)), "%s at time256 %d" % (what, tt)
    # the clamp was exercised on both sides, and ties of zeros of either sign gave the second operand
    lo, hi = np.minimum(dF, dB), np.maximum(dF, dB)
    assert ((dBB < lo).any() and (dBB > hi).any() and ((dBB >= lo) & (dBB <= hi)).any())
