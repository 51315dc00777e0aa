"""CPU tests of mv.DegrainN's creation (it touches no device): the messages -- mvx_degrain_create's texts and order of checks under the
name DegrainN, the radius limit and the overflow text for thsad2 / thsadc2 --, the table of thresholds per temporal distance that info()
reports, and csrc/mvx_degrain_n_weights.h (the header the device code takes its weight arithmetic from) as a stand-alone host program
against the Python restatement (tests/degrain_n_ref.py)."""
import math
import os
import subprocess

import numpy as np
import pytest

import degrain_n_ref
import vector_fields
from test_block_host import INT_MAX, PITCH, _clips, _copy, _err, _scaled_thscd1, _split_uv_pitch

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vapoursynth-mvtools_amd", "csrc")
OVERFLOW = "DegrainN: with this block size and video format, thsad%s must not exceed %d or some calculations would overflow."


def _dn(mv, sup, ad, radius=1, pitch=PITCH, **kw):
    return mv.DegrainN(radius, sup, ad, pitch, **kw)


def test_binding_reaches_radius_24(mv):
    assert mv.DEGRAIN_N_MAX_RADIUS == 24
    sup, bw, _ = _clips(mv)
    assert _dn(mv, sup, bw, radius=24).info()["nrefs"] == 48


def test_argument_checks_are_degrains_in_degrains_order(mv):
    sup, bw, _ = _clips(mv)
    radius = "DegrainN: radius must be between 1 and 24."
    assert _err(lambda: _dn(mv, sup, bw, radius=0)) == radius
    assert _err(lambda: _dn(mv, sup, bw, radius=25, plane=9)) == radius
    assert _err(lambda: _dn(mv, sup, bw, radius=-3)) == radius
    _dn(mv, sup, bw, radius=1)
    _dn(mv, sup, bw, radius=24)
    assert _err(lambda: _dn(mv, sup, bw, plane=5)) == "DegrainN: plane must be between 0 and 4 (inclusive)."
    assert _err(lambda: _dn(mv, sup, bw, radius=9, plane=-1, thscd1=99999)) == "DegrainN: plane must be between 0 and 4 (inclusive)."
    assert _err(lambda: _dn(mv, sup, bw, radius=12, thscd1=16321)) == "DegrainN: thscd1 can be at most 16320."
    _dn(mv, sup, bw, thscd1=16320)
    # thscd1 before the thsad overflow, the overflow before the frame size, the size before the limits
    assert _err(lambda: _dn(mv, sup, bw, thscd1=16321, thsad=1 << 40)) == "DegrainN: thscd1 can be at most 16320."
    sup2 = mv.Super(336, 192, 8)
    assert _err(lambda: _dn(mv, sup2, bw)) == "DegrainN: wrong source or super clip frame size."
    assert _err(lambda: _dn(mv, sup2, bw, thsad=1 << 40)).startswith("DegrainN: with this block size and video format, thsad must")
    assert _err(lambda: _dn(mv, sup2, bw, radius=8, thsad2=1 << 40)).startswith("DegrainN: with this block size and video format, thsad2 must")
    assert _err(lambda: _dn(mv, sup2, bw, limit=256)) == "DegrainN: wrong source or super clip frame size."
    assert _err(lambda: _dn(mv, mv.Super(320, 192, 8, pel=4), bw)) == "DegrainN: wrong source or super clip frame size."
    assert _err(lambda: _dn(mv, mv.Super(320, 200, 8), bw)) == "DegrainN: wrong source or super clip frame size."
    assert _err(lambda: _dn(mv, sup, bw, radius=24, limit=256)) == "DegrainN: limit must be between 0 and 255 (inclusive)."
    assert _err(lambda: _dn(mv, sup, bw, limit=-1, limitc=999)) == "DegrainN: limit must be between 0 and 255 (inclusive)."
    assert _err(lambda: _dn(mv, sup, bw, limitc=256)) == "DegrainN: limitc must be between 0 and 255 (inclusive)."
    assert _err(lambda: _dn(mv, sup, bw, limitc=-1)) == "DegrainN: limitc must be between 0 and 255 (inclusive)."
    _dn(mv, sup, bw, limit=255, limitc=0)
    sup16, bw16, _ = _clips(mv, bits=16)
    assert _err(lambda: _dn(mv, sup16, bw16, pitch=[640, 320, 320], limit=65536)) == "DegrainN: limit must be between 0 and 65535 (inclusive)."
    # the library's own checks come last
    supo, bwo, _ = _clips(mv, overlap=4)
    assert _err(lambda: _dn(mv, supo, _copy(mv, bwo, nBlkX=2))) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: _dn(mv, supo, _copy(mv, bwo, nBlkY=2), limitc=256)) == "DegrainN: limitc must be between 0 and 255 (inclusive)."
    assert _err(lambda: _dn(mv, _split_uv_pitch(mv.Super(320, 192, 8)), bw)) == "U and V super planes must share one pitch."
    assert _err(lambda: _dn(mv, _split_uv_pitch(mv.Super(320, 192, 8)), _copy(mv, bwo, nBlkX=2))) == \
        "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    # Degrain itself keeps its limit and its text
    assert _err(lambda: mv.Degrain(7, sup, bw, PITCH)) == "Degrain: radius must be between 1 and 6."


@pytest.mark.parametrize("bits,thscd1", [(16, None), (16, 200), (10, 37)])
def test_overflow_names_the_argument_at_fault(mv, bits, thscd1):
    """MVDegrains.cpp:658-666 for four arguments: thsad, thsadc, then thsad2, thsadc2; the maximum is INT_MAX * nSCD1_old / nSCD1"""
    sup, bw, _ = _clips(mv, bits=bits, blksize=16)
    old = 400 if thscd1 is None else thscd1
    new = _scaled_thscd1(bw, old)
    maximum = INT_MAX * old // new
    over, ok, pitch = maximum + 2, maximum - 1, [640, 320, 320]
    assert over * new // old >= INT_MAX > ok * new // old
    make = lambda **kw: mv.DegrainN(8, sup, bw, pitch, thscd1=thscd1, **kw)
    assert _err(lambda: make(thsad=over)) == OVERFLOW % ("", maximum)          # (thsadc, thsad2 and thsadc2 follow thsad: the first is named)
    assert _err(lambda: make(thsad=400, thsadc=over)) == OVERFLOW % ("c", maximum)
    assert _err(lambda: make(thsad=400, thsad2=over)) == OVERFLOW % ("2", maximum)     # thsad2 alone
    assert _err(lambda: make(thsad=400, thsadc2=over)) == OVERFLOW % ("c2", maximum)   # thsadc2 alone
    assert _err(lambda: make(thsad=400, thsad2=over, thsadc2=over)) == OVERFLOW % ("2", maximum)
    assert _err(lambda: make(thsad=400, thsadc=over, thsad2=over)) == OVERFLOW % ("c", maximum)
    assert _err(lambda: make(thsad=over, thsad2=100, thsadc=400)) == OVERFLOW % ("", maximum)
    info = make(thsad=ok, thsadc=ok, thsad2=ok, thsadc2=ok).info()
    assert info["thsad_d"] == [ok * new // old] * 8 == info["thsadc_d"]
    # radius 1 has one distance, and thsad2 plays no part in it
    assert mv.DegrainN(1, sup, bw, pitch, thscd1=thscd1, thsad2=over).info()["thsad_d"] == [400 * new // old]


def _formula(t1, t2, radius, d):
    if radius == 1 or t1 == t2:
        return t1
    return int(math.floor(t2 + (t1 - t2) * (1 + math.cos(math.pi * (d - 1) / (radius - 1))) / 2 + 0.5))


@pytest.mark.parametrize("radius", [1, 2, 7, 24])
@pytest.mark.parametrize("bits,akw,thscd1", [(8, dict(blksize=8), None), (16, dict(blksize=16, overlap=8), 300), (10, dict(blksize=32, blksizev=16), None)])
def test_info_reports_the_table_of_thresholds(mv, radius, bits, akw, thscd1):
    sup, bw, _ = _clips(mv, bits=bits, **akw)
    pitch = [640, 320, 320]
    t1, t2, t1c, t2c = 1200, 301, 777, 50
    far = {} if radius == 1 else dict(thsad2=t2, thsadc2=t2c)
    info = mv.DegrainN(radius, sup, bw, pitch, thsad=t1, thsadc=t1c, thscd1=thscd1, **far).info()
    assert (info["radius"], info["nrefs"]) == (radius, 2 * radius)
    old = 400 if thscd1 is None else thscd1
    norm = lambda t: vector_fields.scaled_thresholds(bw, t, old)[0]   # what Degrain scales a thsad to (MVDegrains.cpp:658-659)
    assert norm(400) == 400 * _scaled_thscd1(bw, old) // old
    for table, a, b in ((info["thsad_d"], t1, t2), (info["thsadc_d"], t1c, t2c)):
        assert len(table) == radius
        assert table[0] == norm(a)
        if radius > 1:
            assert table[-1] == norm(b)
        assert all(x >= y for x, y in zip(table, table[1:]))                                  # monotone: falling with the distance
        assert radius < 3 or len(set(table)) >= min(radius, 6)                                # ... and really falling
        for d in range(1, radius + 1):
            f = _formula(a, b, radius, d)
            assert norm(f - 1) <= table[d - 1] <= norm(f + 1), (d, table[d - 1], f)           # libm and Python may differ in the cosine's last place
    # a rising table is legal too
    up = mv.DegrainN(max(radius, 2), sup, bw, pitch, thsad=100, thsad2=400).info()["thsad_d"]
    assert up[0] == norm(100) and up[-1] == norm(400) and all(x <= y for x, y in zip(up, up[1:]))


@pytest.mark.parametrize("radius", [1, 6, 24])
def test_without_thsad2_the_table_is_constant(mv, radius):
    sup, bw, _ = _clips(mv, bits=16, blksize=16)
    info = mv.DegrainN(radius, sup, bw, [640, 320, 320], thsad=350, thsadc=120).info()
    assert info["thsad_d"] == [vector_fields.scaled_thresholds(bw, 350)[0]] * radius
    assert info["thsadc_d"] == [vector_fields.scaled_thresholds(bw, 120)[0]] * radius
    same = mv.DegrainN(radius, sup, bw, [640, 320, 320], thsad=350, thsadc=120, thsad2=350, thsadc2=120).info()
    assert same == info
    # thsadc follows thsad, thsadc2 follows thsadc -- not thsad2
    info = mv.DegrainN(radius, sup, bw, [640, 320, 320], thsad=350, thsad2=100).info()
    assert info["thsadc_d"] == [vector_fields.scaled_thresholds(bw, 350)[0]] * radius


# ------------------------------------------------------------------------------------------------ the weight header as a host program

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("degrain_n_host") / "degrain_n_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           os.path.join(HERE, "degrain_n_host_main.cpp"), "-o", exe])
    return exe


def _ask(exe, tmp_path, lines):
    f = tmp_path / "commands.txt"
    f.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = r.stdout.strip().split("\n")
    assert out[-1] == "degrain_n_host_main: ok" and len(out) == len(lines) + 1
    return [[int(v) for v in l.split()] for l in out[:-1]]


def _weight_cases():
    """(thresholds per reference, usable flags, SADs)"""
    rng = np.random.default_rng(5)
    cases = []
    for n in (2, 4, 6, 8, 14, 16, 18, 24, 48):        # random SADs around a falling table
        for _ in range(40):
            th = np.repeat(np.sort(rng.integers(50, 5000, n // 2))[::-1], 2)
            sad = rng.integers(0, 6000, n)
            cases.append((th, rng.random(n) < 0.85, sad))
    for n in (2, 14, 48):
        th = np.repeat(np.linspace(2400, 600, n // 2).astype(np.int64), 2)
        cases.append((th, np.ones(n, bool), th.copy()))                  # SAD equal to the threshold: weight 0 everywhere
        cases.append((th, np.ones(n, bool), th - 1))                     # one below: the smallest weights
        cases.append((th, np.ones(n, bool), np.zeros(n, np.int64)))      # SAD 0 on every reference (48: every weight 5, WSrc 16)
        cases.append((th, np.zeros(n, bool), np.zeros(n, np.int64)))     # nothing usable
        big = np.full(n, INT_MAX - 1, np.int64)                          # the largest legal threshold
        cases.append((big, np.ones(n, bool), rng.integers(0, INT_MAX - 1, n)))
        cases.append((big, np.ones(n, bool), np.zeros(n, np.int64)))
        cases.append((big, np.ones(n, bool), big - 1))
        cases.append((th, np.ones(n, bool), np.full(n, vector_fields.SAD_HIGH, np.int64)))  # a SAD whose high dword is set
    return cases


def test_host_program_agrees_with_the_restatement_on_weights(host_program, tmp_path):
    cases = _weight_cases()
    lines = ["weights %d %s %s %s" % (len(th), " ".join(str(int(v)) for v in th), " ".join(str(int(v)) for v in ok), " ".join(str(int(v)) for v in sad))
             for th, ok, sad in cases]
    got = _ask(host_program, tmp_path, lines)
    for (th, ok, sad), g in zip(cases, got):
        wsrc, wrefs = degrain_n_ref.normalise(degrain_n_ref.degrain_weights(th, sad) * ok)
        assert g == [int(wsrc)] + [int(w) for w in wrefs], (th, ok, sad)
        assert sum(g) == 256
    # the figures the GPU test of identical frames relies on
    th, ok, sad = np.repeat(np.linspace(2400, 600, 24).astype(np.int64), 2), np.ones(48, bool), np.zeros(48, np.int64)
    wsrc, wrefs = degrain_n_ref.normalise(degrain_n_ref.degrain_weights(th, sad) * ok)
    assert int(wsrc) == 16 and set(int(w) for w in wrefs) == {5}
    # and the scalar DegrainWeight the other vector tests use agrees where nothing wraps
    for th, ok, sad in cases[:50]:
        raw = [vector_fields.degrain_weight(t, s) * int(o) for t, s, o in zip(th, sad, ok)]
        assert raw == [int(w) for w in degrain_n_ref.degrain_weights(th, sad) * ok]


def test_host_program_builds_the_table_creation_reports(mv, host_program, tmp_path):
    sup, bw, _ = _clips(mv, bits=16, blksize=16)
    old, new = 400, _scaled_thscd1(bw, 400)
    asks = [(1200, 300, 24), (400, 100, 8), (400, 400, 7), (1000, 1, 2), (100, 900, 12), (55, 54, 1)]
    got = _ask(host_program, tmp_path, ["table %d %d %d %d %d" % (a, b, r, new, old) for a, b, r in asks])
    for (a, b, r), g in zip(asks, got):
        assert g[0] == 0 and g[1:] == mv.DegrainN(r, sup, bw, [640, 320, 320], thsad=a, thsad2=b).info()["thsad_d"]
    assert _ask(host_program, tmp_path, ["table %d 100 4 %d %d" % (INT_MAX, new, old)])[0][0] == 1
