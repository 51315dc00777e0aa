"""The window arithmetic of the VapourSynth shell's look-ahead engine (vsplugin/mvx_vs_window.h) without a device: a stand-alone C program
(tests/vs_window_main.c, its own main) compiled here with -fsanitize=address,undefined checks the default window length of mv.AnalyseN, the input
ranges at both clip ends and with a radius above the window length, the memory budget and the slot arithmetic against values worked out by hand.
And: the look-ahead windows of mv.AnalyseN change no function list."""
import os
import subprocess

import test_vs_multi_shell as ms
import test_vs_shim as shim
from test_vs_shim import ROOT

VSDIR = os.path.join(ROOT, "vapoursynth-mvtools_amd", "vsplugin")


def test_window_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "vs_window_main")
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I" + VSDIR, os.path.join(ROOT, "tests", "vs_window_main.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)   # (the runtimes are linked in: the program starts in any environment)
    assert r.returncode == 0 and r.stdout.strip() == "OK" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_function_lists_are_unchanged(monkeypatch):
    for s in ms.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for extra in ({}, {"MVX_VS_MULTI_LOOKAHEAD": "4"}, {"MVX_VS_MULTI_LOOKAHEAD": "0"}):
        for k, v in extra.items():
            monkeypatch.setenv(k, v)
        monkeypatch.delenv("MVX_VS_MULTI", raising=False)
        assert ms._listed() == shim.EXPECTED
        monkeypatch.setenv("MVX_VS_MULTI", "1")
        assert ms._listed() == dict(shim.EXPECTED, **ms.NEW)
