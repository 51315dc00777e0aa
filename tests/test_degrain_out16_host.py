"""CPU tests of mv.DegrainN's out16 creation (mvx_degrain_n_create_out16 touches no device): the new message, the limits in units of the
output, out_bits for objects of both create functions, the default pitches of the 16-bit planes, and the threshold tables, which are those of
the 8-bit object -- the vectors, their SADs and every threshold stay in 8-bit units.  out16 adds no host arithmetic to a header, so there is no
stand-alone host program here (tests/degrain_n_host_main.cpp covers csrc/mvx_degrain_n_weights.h, which is unchanged)."""
import pytest

from test_block_host import PITCH, _clips, _err

NEEDS_8 = "DegrainN: out16 needs an 8 bit clip."


def _dn(mv, sup, ad, radius=1, pitch=PITCH, **kw):
    return mv.DegrainN(radius, sup, ad, pitch, **kw)


@pytest.mark.parametrize("bits", [10, 16])
def test_out16_refuses_a_super_clip_that_is_not_8_bit(mv, bits):
    sup, bw, _ = _clips(mv, bits=bits)
    pitch = [640, 320, 320]
    assert _err(lambda: _dn(mv, sup, bw, pitch=pitch, out16=True)) == NEEDS_8
    assert _err(lambda: _dn(mv, sup, bw, radius=24, pitch=pitch, out16=True, limit=70000)) == NEEDS_8   # before the limits, whose range it decides
    assert _dn(mv, sup, bw, pitch=pitch).out_bits == bits                                               # without out16: the clip's depth
    # the checks that come before it keep their place
    assert _err(lambda: _dn(mv, sup, bw, radius=25, pitch=pitch, out16=True)) == "DegrainN: radius must be between 1 and 24."
    assert _err(lambda: _dn(mv, sup, bw, plane=5, pitch=pitch, out16=True)) == "DegrainN: plane must be between 0 and 4 (inclusive)."
    assert _err(lambda: _dn(mv, mv.Super(336, 192, bits), bw, pitch=pitch, out16=True)) == "DegrainN: wrong source or super clip frame size."


def test_limits_are_in_units_of_the_output(mv):
    sup, bw, _ = _clips(mv)
    limit, limitc = "DegrainN: limit must be between 0 and 65535 (inclusive).", "DegrainN: limitc must be between 0 and 65535 (inclusive)."
    _dn(mv, sup, bw, out16=True, limit=65535)
    _dn(mv, sup, bw, out16=True, limit=65535, limitc=65535)
    _dn(mv, sup, bw, out16=True, limit=0, limitc=0)
    _dn(mv, sup, bw, out16=True, limit=256)    # one step of the 8-bit clip: refused without out16
    assert _err(lambda: _dn(mv, sup, bw, out16=True, limit=65536)) == limit
    assert _err(lambda: _dn(mv, sup, bw, out16=True, limit=-1)) == limit
    assert _err(lambda: _dn(mv, sup, bw, out16=True, limitc=65536)) == limitc
    assert _err(lambda: _dn(mv, sup, bw, out16=True, limit=300, limitc=-1)) == limitc
    assert _err(lambda: _dn(mv, sup, bw, out16=True, limit=-1, limitc=99999)) == limit
    # the 8-bit object keeps its own range and text
    assert _err(lambda: _dn(mv, sup, bw, limit=256)) == "DegrainN: limit must be between 0 and 255 (inclusive)."
    assert _err(lambda: _dn(mv, sup, bw, out16=False, limitc=256)) == "DegrainN: limitc must be between 0 and 255 (inclusive)."
    # the other messages are mvx_degrain_n_create's
    assert _err(lambda: _dn(mv, sup, bw, out16=True, radius=0)) == "DegrainN: radius must be between 1 and 24."
    assert _err(lambda: _dn(mv, sup, bw, out16=True, thscd1=16321)) == "DegrainN: thscd1 can be at most 16320."
    assert _err(lambda: _dn(mv, mv.Super(336, 192, 8), bw, out16=True)) == "DegrainN: wrong source or super clip frame size."
    supo, bwo, _ = _clips(mv, overlap=4)
    from test_block_host import _copy
    assert _err(lambda: _dn(mv, supo, _copy(mv, bwo, nBlkX=2), out16=True)) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."


def test_out_bits_and_default_pitches(mv):
    sup, bw, _ = _clips(mv)
    new, old = _dn(mv, sup, bw, out16=True), _dn(mv, sup, bw)
    assert (new.out_bits, old.out_bits) == (16, 8)          # an object of mvx_degrain_n_create still reports 8
    assert _dn(mv, sup, bw, radius=24, out16=False).out_bits == 8
    assert (new.out16, old.out16) == (True, False)
    assert old.dst_pitch == PITCH and new.src_pitch == PITCH
    assert new.dst_pitch == [768, 512, 512]                 # rows of 320 / 160 16-bit samples, rounded up to 256 bytes
    assert _dn(mv, sup, bw, out16=True, dst_pitch=[640, 320, 320]).dst_pitch == [640, 320, 320]
    gsup = mv.Super(320, 192, 8, gray=True)
    assert _dn(mv, gsup, bw, pitch=[320], out16=True).dst_pitch == [768]


@pytest.mark.parametrize("radius", [1, 7, 24])
@pytest.mark.parametrize("akw,thscd1", [(dict(blksize=8), None), (dict(blksize=16, overlap=8), 300), (dict(blksize=32, blksizev=16), None)])
def test_threshold_tables_are_the_8_bit_objects(mv, radius, akw, thscd1):
    sup, bw, _ = _clips(mv, **akw)
    far = {} if radius == 1 else dict(thsad2=301, thsadc2=50)
    kw = dict(thsad=1200, thsadc=777, thscd1=thscd1, **far)
    new, old = _dn(mv, sup, bw, radius=radius, out16=True, **kw).info(), _dn(mv, sup, bw, radius=radius, **kw).info()
    assert new == old and len(new["thsad_d"]) == radius
    assert radius == 1 or new["thsad_d"][0] > new["thsad_d"][-1]
    # and the limits play no part in them
    assert _dn(mv, sup, bw, radius=radius, out16=True, limit=4000, limitc=0, **kw).info() == old
