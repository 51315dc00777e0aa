"""Deep mv.Mask through the VapourSynth filter shell: with MVX_VS_MASK_DEEP=1 beside MVX_VS_FLOW=1 in the host's environment, mv.Mask takes
clips of 9 to 16 bits and gives a mask clip of the clip's depth.  Whole graphs -- Super -> Analyse -> Mask -- run through the mini host, one
process per case, against tests/mask_deep_ref.py fed the CPU oracle's blobs; the cases take no pow (kinds 1 and 2 at gamma 1, kind 5), where
the library is exact.  The mini host writes frames in the output node's own format and prints it."""
import math

import numpy as np
import pytest

import mask_deep_ref
import mask_ref
from test_vs_flow_shell import Graph, _fkw, _same

pytestmark = pytest.mark.gpu

DEEP_FORMAT = "Mask: input clip must be Gray or YUV (4:2:0, 4:2:2, 4:4:0, 4:4:4) of 8 to 16 bits, with constant dimensions."


@pytest.fixture
def deep_on(monkeypatch):
    monkeypatch.setenv("MVX_VS_FLOW", "1")  # (proc_env() copies os.environ)
    monkeypatch.setenv("MVX_VS_MASK_DEEP", "1")


def _expected(g, fargs, fw):
    an, blobs = (g.afw, g.bfw) if fw else (g.abw, g.bbw)
    ref = mask_deep_ref.DeepMask(an.ad, g.bits, **_fkw(fargs))
    stats = {}
    want = [ref.frame(blobs[n], g.frames[n][0], stats) for n in range(g.nf)]
    assert ref.pow_dist == math.inf, "the case takes a pow: not exact by construction"
    return want, ref, ",".join(sorted(k for k, v in stats.items() if v > 0))


CASES = [
    # w, h, bits, fmt, forward vectors, filter arguments, the restatement's counters, the mask clip's format as the mini host prints it
    (128, 96, 16, "420", False, dict(kind=1), "sc", "family=yuv bits=16 bytes=2 ssw=1 ssh=1 planes=3"),
    (128, 96, 10, "444", True, dict(kind=5, ml="3.0"), "cut,sc", "family=yuv bits=10 bytes=2 ssw=0 ssh=0 planes=3"),       # the luma kept at 10 bits
    (128, 96, 12, "gray", False, dict(kind=2, ysc=77), "sc", "family=yuv bits=12 bytes=2 ssw=0 ssh=0 planes=3"),             # Gray in, 4:4:4 out
    (206, 118, 16, "420", True, dict(kind=5, ysc=200), "edgex,edgey,sc", "family=yuv bits=16 bytes=2 ssw=1 ssh=1 planes=3"),
]


@pytest.mark.parametrize("w,h,bits,fmt,fw,fargs,counters,vi", CASES, ids=["%dx%d-%s-b%d-k%d" % (c[0], c[1], c[3], c[2], c[5]["kind"]) for c in CASES])
def test_deep_mask_graph_matches_restatement(deep_on, oracle, tmp_path, w, h, bits, fmt, fw, fargs, counters, vi):
    g = Graph(oracle, tmp_path, w, h, bits, 4, fmt, seed=71)
    want, ref, seen = _expected(g, fargs, fw)
    assert seen == counters
    if fargs["kind"] == 1:
        assert 2 * ref.shifted >= ref.cells > 0
    r, path = g.run("mask", fargs, *(["x.vectors=fw"] if fw else []))
    assert "mask format " + vi in r.stdout.splitlines()
    _same(g.read(path, g.nf, bits=bits, fmt="444" if fmt == "gray" else fmt), want, "Mask")


def test_an_8_bit_graph_is_unchanged_by_the_switch(deep_on, oracle, tmp_path, monkeypatch):
    g = Graph(oracle, tmp_path, 206, 118, 8, 4, seed=71)
    fargs = dict(kind=5, ysc=77)
    ref = mask_ref.Mask(g.abw.ad, **fargs)
    want = [ref.frame(g.bbw[n], g.frames[n][0], {}) for n in range(g.nf)]
    r, path = g.run("mask", fargs, name="deep.raw")
    assert "mask format family=yuv bits=8 bytes=1 ssw=1 ssh=1 planes=3" in r.stdout.splitlines()
    _same(g.read(path, g.nf), want, "Mask with the switch")
    monkeypatch.delenv("MVX_VS_MASK_DEEP")
    r, plain = g.run("mask", fargs, name="plain.raw")
    assert "mask format family=yuv bits=8 bytes=1 ssw=1 ssh=1 planes=3" in r.stdout.splitlines()
    assert open(path, "rb").read() == open(plain, "rb").read()


def test_the_switch_alone_registers_nothing(oracle, tmp_path, monkeypatch):
    """MVX_VS_MASK_DEEP is effective only where mv.Mask is registered at all"""
    monkeypatch.delenv("MVX_VS_FLOW", raising=False)
    monkeypatch.setenv("MVX_VS_MASK_DEEP", "1")
    g = Graph(oracle, tmp_path, 128, 96, 16, 3, seed=71)
    r, _ = g.run("mask", dict(kind=1), check=False)
    assert "DONE" not in r.stdout and "ERROR mask: no function Mask" in r.stdout
