"""CPU tests of the float BlockFPS entry (mvx_blockfps_create_float; no create touches a device and mvx_blockfps_frames checks its jobs before any
launch): every creation message in its order with the two float-specific ones, the integer create's refusal, pitches and job layouts at a sample
size of 4, get_info / map against the integer object's, the package's sample_float keyword -- and csrc/mvx_blockfps_float_rule.h as a
stand-alone host program (with AddressSanitizer and UBSan where g++ links them) against tests/blockfps_float_ref.py, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import blockfps_float_ref as bf
from test_block_host import _clips, _copy, _err, _split_uv_pitch
from test_float_host import CSRC, HERE, _sanitizer_flags

FPITCH = [1280, 640, 640]  # rows of 320 / 160 float samples


def _fsup(mv, w=320, h=192, **kw):
    return mv.Super(w, h, 32, sample_float=True, **kw)


def _b(mv, sup, bw, fw, fps=(24, 1), pitch=FPITCH, **kw):
    return mv.BlockFPS(sup, bw, fw, 10, pitch, fps[0], fps[1], sample_float=True, **kw)


def test_float_blockfps_messages_and_their_order(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    size = "BlockFPS: wrong source or super clip frame size."
    needs = "BlockFPS: the float entry needs a float super clip."
    rate = "BlockFPS: The input clip must have a frame rate. Invoke AssumeFPS if necessary."
    _b(mv, fsup, bw, fw)
    for mode in range(9):
        assert _b(mv, fsup, bw, fw, mode=mode).is_float
    assert _err(lambda: _b(mv, fsup, bw, fw, mode=9)) == "BlockFPS: mode must be between 0 and 8 (inclusive)."
    assert _err(lambda: _b(mv, fsup, bw, fw, mode=-1, thscd1=99999)) == "BlockFPS: mode must be between 0 and 8 (inclusive)."
    assert _err(lambda: _b(mv, isup, bw, fw, mode=9)) == "BlockFPS: mode must be between 0 and 8 (inclusive)."    # (before the kind of super clip)
    assert _err(lambda: _b(mv, fsup, bw, fw, thscd1=16321)) == "BlockFPS: thscd1 can be at most 16320."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nWidth=336), thscd1=16321)) == "BlockFPS: thscd1 can be at most 16320."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nWidth=336))) == "BlockFPS: mvbw and mvfw have different widths."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nHeight=200))) == "BlockFPS: mvbw and mvfw have different heights."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nBlkSizeX=16))) == "BlockFPS: mvbw and mvfw have different block sizes."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nBlkSizeY=16))) == "BlockFPS: mvbw and mvfw have different block sizes."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nPel=4))) == "BlockFPS: mvbw and mvfw have different pel precision."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nOverlapX=2))) == "BlockFPS: mvbw and mvfw have different overlap."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nOverlapY=2))) == "BlockFPS: mvbw and mvfw have different overlap."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nWidth=336, nPel=4))) == "BlockFPS: mvbw and mvfw have different widths."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nPel=4, nDeltaFrame=0))) == "BlockFPS: mvbw and mvfw have different pel precision."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nDeltaFrame=0))) == "BlockFPS: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _b(mv, fsup, bw, _copy(mv, fw, nDeltaFrame=2))) == "BlockFPS: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _b(mv, fsup, fw, fw)) == "BlockFPS: mvbw must be generated with isb=True."
    assert _err(lambda: _b(mv, fsup, bw, bw)) == "BlockFPS: mvfw must be generated with isb=False."
    assert _err(lambda: _b(mv, fsup, bw, bw, fps=(0, 1))) == "BlockFPS: mvfw must be generated with isb=False."
    assert _err(lambda: _b(mv, fsup, bw, fw, fps=(0, 1))) == rate
    assert _err(lambda: _b(mv, fsup, bw, fw, fps=(24, 0))) == rate
    assert _err(lambda: _b(mv, _fsup(mv, w=336), bw, fw)) == size
    assert _err(lambda: _b(mv, _fsup(mv, w=336), bw, fw, fps=(0, 1))) == rate
    assert _err(lambda: _b(mv, _fsup(mv, pel=4), bw, fw)) == size
    assert _err(lambda: _b(mv, _fsup(mv, h=200), bw, fw)) == size
    # an integer super clip handed to the float entry: after the frame size, before the library's own geometry and pitch checks
    assert _err(lambda: _b(mv, isup, bw, fw)) == needs
    assert _err(lambda: _b(mv, isup, bw, fw, fps=(0, 1))) == rate
    assert _err(lambda: _b(mv, mv.Super(336, 192, 8), bw, fw)) == size
    sup16, bw16, fw16 = _clips(mv, bits=16)
    assert _err(lambda: _b(mv, sup16, bw16, fw16)) == needs
    assert _err(lambda: _b(mv, _split_uv_pitch(mv.Super(320, 192, 8)), bw, fw)) == needs
    assert _err(lambda: _b(mv, isup, bw, fw, pitch=[2, 2, 2])) == needs
    _b(mv, fsup, bw16, fw16)                                          # vectors of a 16-bit search
    _, bwo, fwo = _clips(mv, overlap=4)
    assert _err(lambda: _b(mv, fsup, _copy(mv, bwo, nBlkX=2), _copy(mv, fwo, nBlkX=2))) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: _b(mv, _split_uv_pitch(_fsup(mv)), bw, fw)) == "U and V super planes must share one pitch."
    # the integer entry keeps its refusal, first of all
    assert _err(lambda: mv.BlockFPS(fsup, bw, fw, 10, FPITCH, mode=77)) == "BlockFPS: float super clips are not supported."
    assert _err(lambda: mv.BlockFPS(fsup, bw, _copy(mv, fw, nWidth=336), 10, FPITCH, 0, 1)) == "BlockFPS: float super clips are not supported."


def test_pitches_of_the_float_entry(mv):
    """clip and dst: any pitch that holds a row and is a multiple of 4; super: multiples of 16"""
    _, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    rows = [320 * 4, 160 * 4, 160 * 4]
    msg = lambda what, p: "%s pitch of plane %d must hold a row of %d bytes and be a multiple of the sample size." % (what, p, rows[p])
    assert _b(mv, fsup, bw, fw, pitch=rows).dst_pitch == rows
    _b(mv, fsup, bw, fw, pitch=[rows[0] + 4, rows[1], rows[2] + 256])                  # an odd multiple of 4; U != V
    assert _b(mv, fsup, bw, fw, pitch=rows, dst_pitch=[2048, 1024, 768]).dst_pitch == [2048, 1024, 768]
    assert _err(lambda: _b(mv, fsup, bw, fw, pitch=[rows[0] + 2, rows[1], rows[2]])) == msg("clip", 0)
    assert _err(lambda: _b(mv, fsup, bw, fw, pitch=[rows[0], rows[1] - 4, rows[2]])) == msg("clip", 1)
    assert _err(lambda: _b(mv, fsup, bw, fw, pitch=rows, dst_pitch=[rows[0], rows[1], rows[2] + 1])) == msg("dst", 2)
    assert _err(lambda: _b(mv, fsup, bw, fw, pitch=[320, 160, 160])) == msg("clip", 0)  # (the integer clip's pitches do not hold a float row)
    odd = _fsup(mv)
    odd.pitch = [odd.pitch[0] + 8, odd.pitch[1], odd.pitch[2]]
    assert _err(lambda: _b(mv, odd, bw, fw)).startswith("super pitch of plane 0 must hold a row of ")


@pytest.mark.parametrize("rate", [dict(num=60, den=1), dict(), dict(num=0, den=0), dict(num=30000, den=1001), dict(num=-5, den=1)], ids=["60", "25", "double", "ntsc", "none"])
@pytest.mark.parametrize("delta", [1, 2])
def test_info_and_map_are_the_integer_objects(mv, rate, delta):
    isup, bw, fw = _clips(mv, delta=delta)
    new, old = _b(mv, _fsup(mv), bw, fw, **rate), mv.BlockFPS(isup, bw, fw, 10, [320, 160, 160], 24, 1, **rate)
    assert (new.num_frames, new.fps_num, new.fps_den) == (old.num_frames, old.fps_num, old.fps_den)
    assert [new.map(n) for n in range(new.num_frames + 2)] == [old.map(n) for n in range(old.num_frames + 2)]
    assert new.is_float and not old.is_float
    if rate == dict(num=60, den=1) and delta == 1:
        assert new.num_frames == 23 and [new.map(n)[2] for n in range(6)] == [0, 102, 205, 51, 154, 0]


def test_frames_checks_its_jobs_before_any_device_call(mv):
    _, bw, fw = _clips(mv)
    L, A = mv.lib(), 0x10000  # never dereferenced
    b = _b(mv, _fsup(mv), bw, fw)
    job = (mv.BlockFPSJob * 2)()

    def fill(left=(A, A, A), right=(A, A, A), dst=(A, A, A), src=(A, A, A), ref=(A, A, A), t=128, k=0):
        for j in range(2):
            job[j].time256 = 128
            for p in range(3):
                job[j].clip_left[p], job[j].clip_right[p], job[j].dst[p], job[j].src_super[p], job[j].ref_super[p] = A, A, A, A, A
        job[k].time256 = t
        for p in range(3):
            job[k].clip_left[p], job[k].clip_right[p], job[k].dst[p], job[k].src_super[p], job[k].ref_super[p] = left[p], right[p], dst[p], src[p], ref[p]
        assert L.mvx_blockfps_frames(b.h, 2, job, None) == -1
        return L.mvx_last_error().decode()
    assert fill(left=(None, A, A)) == "mvx_blockfps_frames: clip_left / clip_right are required"
    assert fill(right=(None, A, A), k=1) == "mvx_blockfps_frames: clip_left / clip_right are required"
    assert fill(left=(A + 2, A, A)) == "mvx_blockfps_frames: clip_left plane 0 must be aligned to 4 bytes"
    assert fill(left=(A, A, None)) == "mvx_blockfps_frames: clip_left plane 2 is required"
    assert fill(right=(A, A + 6, A), k=1) == "mvx_blockfps_frames: clip_right plane 1 must be aligned to 4 bytes"
    assert fill(dst=(A, A, A + 1)) == "mvx_blockfps_frames: dst plane 2 must be aligned to 4 bytes"
    assert fill(dst=(A, None, A), k=1) == "mvx_blockfps_frames: dst plane 1 is required"
    assert fill(src=(A + 4, A, A)) == "mvx_blockfps_frames: source super plane 0 must be aligned to 16 bytes"
    assert fill(ref=(A, A + 8, A), k=1) == "mvx_blockfps_frames: reference super plane 1 must be aligned to 16 bytes"
    assert fill(left=(A + 2, A, A), t=0) == "mvx_blockfps_frames: clip_left plane 0 must be aligned to 4 bytes"
    assert L.mvx_blockfps_frames(b.h, 0, job, None) == 0


def test_the_keyword_selects_the_float_entry_and_nothing_else_changes(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    new, old = _b(mv, fsup, bw, fw), mv.BlockFPS(isup, bw, fw, 10, [320, 160, 160])
    assert new.is_float and not old.is_float and new.dst_pitch == FPITCH and old.dst_pitch == [320, 160, 160]
    assert _err(lambda: mv.BlockFPS(fsup, bw, fw, 10, FPITCH)) == "BlockFPS: float super clips are not supported."
    assert _err(lambda: _b(mv, isup, bw, fw)) == "BlockFPS: the float entry needs a float super clip."
    assert np.dtype(fsup.dtype) == np.float32


# ------------------------------------------------------------------------------------------------ the rule header on the host

@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    assert shutil.which("g++"), "the host program needs g++"
    tmp = str(tmp_path_factory.mktemp("blockfps_float_rule"))
    exe = os.path.join(tmp, "blockfps_float_rule_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + CSRC, os.path.join(HERE, "blockfps_float_rule_host_main.cpp"),
                           "-o", exe] + _sanitizer_flags(tmp))
    return exe


MASKS = (0, 1, 127, 254, 255)


@pytest.mark.parametrize("mode", range(9))
def test_rule_header_on_the_host_is_the_restatement(rule_exe, mode):
    """every time256 1..255 against every triple of masks at 0 / 1 / 127 / 254 / 255, random samples -- luma-like, chroma-like (negative) and
    overshooting, a few equal and a few zeros of either sign for the median -- and random window weights: bit for bit tests/blockfps_float_ref.py"""
    rng = np.random.default_rng(700 + mode)
    t, mF, mB, mO = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(1, 256), MASKS, MASKS, MASKS, indexing="ij"))
    n = t.size
    f = (rng.random((4, n)) * 1.5 - 0.2).astype(np.float32)
    f[:, ::3] -= np.float32(0.5)
    f[1, ::7] = f[0, ::7]
    f[3, ::11] = f[2, ::11]
    f[0, ::13], f[1, ::26] = np.float32(0.0), np.float32(-0.0)
    w = rng.integers(1, 2049, (4, n)).astype(np.int32)
    k = np.concatenate([np.stack([mF, mB, mO, t]), w]).astype(np.int32)
    r = subprocess.run([rule_exe, str(mode), str(n)], input=f.tobytes() + k.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    out = np.frombuffer(r.stdout, np.float32).reshape(3, n)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    tt = t.astype(np.int64)
    ft, fu = tt.astype(np.float32), (256 - tt).astype(np.float32)
    time_ = lambda right, left: (right * ft + left * fu) * bf.K
    s, rr, b, fw = f

    def value():
        mix = bf.mix
        if mode == 0:
            return time_(b, fw)
        if mode == 1:
            return bf.med(rr, s, time_(b, fw))
        if mode == 2:
            return bf.med(time_(rr, s), b, fw)
        if mode in (3, 6):
            return time_(mix(mB, fw, b), mix(mF, b, fw))
        if mode in (4, 7):
            return mix(mO, time_(rr, s), time_(mix(mB, fw, b), mix(mF, b, fw)))
        return mO.astype(np.float32) / np.float32(255.0)
    v = value()
    assert v.dtype == np.float32 and np.array_equal(bits(out[0]), bits(v)), "mode %d" % mode
    assert np.array_equal(bits(out[1]), bits(time_(rr, s)))
    acc = np.zeros(n, np.float32)
    for term, wk in zip((v, s, rr, b), w):
        acc = acc + term * wk.astype(np.float32)
    assert np.array_equal(bits(out[2]), bits(acc / w.sum(axis=0).astype(np.float32)))
    # the vectorised expressions above are blockfps_float_ref's own functions at one time per sample
    one = slice(0, 125)
    assert np.array_equal(bits(bf.value(mode, 1, s[one], rr[one], b[one], fw[one], mF[one], mB[one], mO[one])), bits(v[one]))
