"""CPU tests around the dct 1..4 cost modes: the DCT-capable oracle built at test time (tests/dct_oracle.py) changes nothing but those modes; the
switch mvx_enable_dct_float / mv.enable_dct_float and what both creates say with it off and on; the C header; the VapourSynth shell's MVX_VS_DCT;
csrc/mvx_dct_host.h as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dct_oracle as do
import pipeline as pl
from test_vs_shim import HOST, PLUGIN, host

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vapoursynth-mvtools_amd", "csrc")
OFF_TEXT = "%s: dct 1..4 (FFTW3 DCT cost) are not implemented on the GPU path."


# ------------------------------------------------------------------------------------------------ the patched oracle

def test_every_anchor_of_the_patch_matches_once():
    text = do.patched_source()
    assert text.count("dct_emu_luma_cost(") == 2 and "need FFTW3" not in text
    stock = open(os.path.join(ROOT, "oracle", "mvo_analyse.c")).read()
    assert len(text.splitlines()) == len(stock.splitlines()) - 2 + 3  # two refusals out; the call (two lines) and its prototype in


@pytest.mark.parametrize("dct", [0, 5, 7, 9])
def test_patched_oracle_is_inert_elsewhere(oracle, dct):
    """blobs of the modes the stock oracle has are identical from both (Analyse with a brightness ramp so that 7 and 9 mix, and Recalculate)"""
    od = do.module()
    assert od is not oracle and od.lib() is not oracle.lib()
    w, h, bits = 128, 80, 8
    frames = pl.moving_clip(w, h, bits, 3, seed=11, noise=3)
    frames[1][0][...] = np.clip(frames[1][0].astype(np.int64) + np.linspace(0, 40, w)[None, :].astype(np.int64), 0, 255).astype(np.uint8)
    blobs = []
    for o in (oracle, od):
        sup = o.Super(w, h, bits)
        sf = [sup.frame(f) for f in frames]
        an = o.Analyse(sup, blksize=8, overlap=4, dct=dct)
        b = [an.frame(sf[0], sf[1]), an.frame(sf[1], sf[0]), an.frame(sf[1], sf[2]), an.frame(sf[2], None)]
        rc = o.Recalculate(sup, an.ad, blksize=8, overlap=4, thsad=60, dct=dct)
        b.append(rc.frame(sf[0], sf[1], b[0]))
        blobs.append(b)
    for a, b in zip(*blobs):
        assert np.array_equal(a, b)


def test_patched_oracle_runs_the_float_modes_and_they_differ():
    od = do.module()
    w, h, bits = 128, 80, 8
    frames = pl.moving_clip(w, h, bits, 2, seed=11, noise=3)
    sup = od.Super(w, h, bits)
    sf = [sup.frame(f) for f in frames]
    b0 = od.Analyse(sup, blksize=8, dct=0).frame(sf[0], sf[1])
    b1 = od.Analyse(sup, blksize=8, dct=1).frame(sf[0], sf[1])
    assert b1.shape == b0.shape and not np.array_equal(b0, b1)
    # mode 2 without a brightness change is the spatial search (dctweight16 == 0); so are modes 3 and 4 on a clip so flat that no candidate's luma sum
    # is a 32nd away from the source block's (on the textured clip motion alone moves a block's luma sum further than that)
    assert np.array_equal(od.Analyse(sup, blksize=8, dct=2).frame(sf[0], sf[1]), b0)
    flat = [sup.frame(f) for f in do.flat_clip(frames)]
    f0 = od.Analyse(sup, blksize=8, dct=0).frame(flat[0], flat[1])
    for m in (3, 4):
        assert np.array_equal(od.Analyse(sup, blksize=8, dct=m).frame(flat[0], flat[1]), f0), m
        assert not np.array_equal(od.Analyse(sup, blksize=8, dct=m).frame(sf[0], sf[1]), b0), m


# ------------------------------------------------------------------------------------------------ the switch

def _recalc(mv, sup, **kw):
    return mv.Recalculate(sup, mv.Analyse(sup, blksize=16).ad, **kw)


def test_switch_off_is_today_s_refusal(mv):
    assert mv.enable_dct_float(False) is False  # off by default, and stays off for the rest of the suite
    sup = mv.Super(128, 80, 8)
    for dct in (1, 2, 3, 4):
        with pytest.raises(mv.MvtoolsError) as e:
            mv.Analyse(sup, dct=dct)
        assert str(e.value) == OFF_TEXT % "Analyse"
        with pytest.raises(mv.MvtoolsError) as e:
            _recalc(mv, sup, dct=dct)
        assert str(e.value) == OFF_TEXT % "Recalculate"


def test_switch_round_trips_and_opens_both_creates(mv):
    assert mv.enable_dct_float(True) is False
    try:
        assert mv.enable_dct_float(True) is True
        sup = mv.Super(128, 80, 16)
        for dct in (1, 2, 3, 4):
            for kw in (dict(blksize=4), dict(blksize=8, blksizev=4), dict(blksize=16, blksizev=2), dict(blksize=32)):  # 16x2 is legal here (only 5..10 refuse it)
                assert mv.Analyse(sup, dct=dct, **kw).blob_size > 0
                assert _recalc(mv, sup, dct=dct, **kw).blob_size > 0
        for kw in (dict(blksize=64), dict(blksize=64, blksizev=32)):  # the float DCT builds stop at 32x32, loudly
            with pytest.raises(mv.MvtoolsError) as e:
                mv.Analyse(mv.Super(512, 384, 8), dct=1, **kw)
            assert str(e.value) == "Analyse: dct 1..4 are implemented for blocks up to 32x32."
        with pytest.raises(mv.MvtoolsError) as e:
            mv.Analyse(sup, dct=11)
        assert str(e.value) == "Analyse: dct must be between 0 and 10 (inclusive)."
    finally:
        assert mv.enable_dct_float(False) is True
    with pytest.raises(mv.MvtoolsError):
        mv.Analyse(mv.Super(128, 80, 8), dct=1)


def test_test_entry_refuses_a_handle_without_the_float_modes(mv):
    an = mv.Analyse(mv.Super(128, 80, 8), dct=5)
    rc = mv.lib().mvx_analyse_dct_blocks(an.h, None, 0, 1, (C.c_int32 * 1)(0), (C.c_int32 * 1)(0), None, None)
    assert rc != 0 and b"dct 1..4" in mv.lib().mvx_last_error()


def test_header_declares_the_two_calls(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include "mvtools_amd.h"\n'
                   'int (*a)(int) = mvx_enable_dct_float;\n'
                   'int (*b)(mvx_analyse *, const void *, ptrdiff_t, int, const int32_t *, const int32_t *, void *, void *) = mvx_analyse_dct_blocks;\n')
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "decl.o")])
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vapoursynth-mvtools_amd", "libmvtools_amd.so")], capture_output=True, text=True).stdout
    assert " T mvx_enable_dct_float" in syms and " T mvx_analyse_dct_blocks" in syms


# ------------------------------------------------------------------------------------------------ the VapourSynth shell

def test_shell_forwards_MVX_VS_DCT_once_and_only_then(tmp_path):
    """a test double of the one call (LD_PRELOAD in front of the library) sees it when the host's environment has MVX_VS_DCT=1 as the plugin is
    loaded; without the variable the call is not made, and the registered functions are the same either way"""
    host("list")  # (builds the shell when it is missing)
    dbl = str(tmp_path / "libdct_double.so")
    (tmp_path / "dbl.c").write_text('#include <stdio.h>\nint mvx_enable_dct_float(int on) { fprintf(stderr, "dct_double: enable %d\\n", on); return 0; }\n')
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(tmp_path / "dbl.c"), "-o", dbl])
    outs = {}
    for val in (None, "0", "1"):
        env = dict(os.environ, LD_PRELOAD=(dbl + " " + os.environ.get("LD_PRELOAD", "")).strip())
        env.pop("MVX_VS_DCT", None)
        if val is not None:
            env["MVX_VS_DCT"] = val
        r = subprocess.run([HOST, PLUGIN, "list"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr
        outs[val] = r.stdout
        assert r.stderr.count("dct_double: enable 1") == (1 if val == "1" else 0) and "enable 0" not in r.stderr, r.stderr
    assert outs[None] == outs["0"] == outs["1"]


# ------------------------------------------------------------------------------------------------ sanitizers

def _no_sanitizers(tmp):
    src = os.path.join(tmp, "one.cpp")
    open(src, "w").write("int main() { return 0; }\n")
    if not shutil.which("g++"):
        return "no g++"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", src, "-o", os.path.join(tmp, "one")], capture_output=True)
    return None if r.returncode == 0 and subprocess.run([os.path.join(tmp, "one")]).returncode == 0 else "g++ does not link -fsanitize=address,undefined here"


def test_host_header_under_sanitizers(tmp_path):
    why = _no_sanitizers(str(tmp_path))
    if why:
        pytest.skip(why)
    exe = str(tmp_path / "dct_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "dct_host_main.cpp"), "-o", exe,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "dct_host_main: ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
