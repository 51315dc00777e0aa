"""CPU tests of mvx_depan_compensate_create_float and mvx_depan_stabilise_create_float (no device is touched): the integer entries' messages in
their order with the one new message, for a clip that is not 32-bit, where the format message sits; the pitch rule of 4; the library's own
size checks; the integer entries' unchanged refusal of a 32-bit clip; the contents of info; and the host arithmetic (map, transform, window,
plan) of a float object against an integer object's, which it shares."""
import ctypes as C

import numpy as np
import pytest

W, H = 206, 118
FORMAT = "clip must have constant format and dimensions, integer sample type, bit depth up to 16, and it must be Gray, 420, 422, or 444, and not RGB."
NOT32 = "the float path takes a 32-bit float clip; create an 8..16 bit clip's filter with the integer entry."
SIZE = "every plane must be at least 2 samples wide and 2 high, and the frame at most 32767 x 32767."
PITCH = "pitches must hold a row of their plane and be multiples of the sample size."

# several wrong at once: the earliest in the order wins.  bits=16 stands where bits=32 stands for the integer entries
COMP_ORDER = dict(offset=11.0, subpixel=5, pixaspect=-1.0, mirror=99, blur=-3, bits=16, data_frames=1)
COMP_TEXTS = ["offset must be between -10.0 and 10.0 (inclusive).", "subpixel must be between 0 and 2 (inclusive).", "pixaspect must be greater than 0.",
              "mirror must be between 0 and 15 (inclusive).", "blur must not be negative.", NOT32, "data must have at least as many frames as clip."]
STAB_ORDER = dict(cutoff=0.0, prev=-1, next=-1, subpixel=5, pixaspect=-1.0, mirror=99, blur=-3, method=7, bits=16, fps=(0, 0), data_frames=1)
STAB_TEXTS = ["cutoff must be greater than 0.", "prev must not be negative.", "next must not be negative.", "subpixel must be between 0 and 2 (inclusive).",
              "pixaspect must be greater than 0.", "mirror must be between 0 and 15 (inclusive).", "blur must not be negative.", "method must be between 0 and 1 (inclusive).",
              NOT32, "clip must have known frame rate.", "data must have at least as many frames as clip."]


def comp(mv, w=W, h=H, bits=32, sample_float=True, **kw):
    return mv.DepanCompensate(w, h, bits, sample_float=sample_float, **dict(dict(offset=1.0, num_frames=10), **kw))


def stab(mv, w=W, h=H, bits=32, sample_float=True, **kw):
    return mv.DepanStabilise(w, h, bits, sample_float=sample_float, **dict(dict(num_frames=10), **kw))


@pytest.mark.parametrize("make,name,order,texts", [(comp, "DepanCompensate", COMP_ORDER, COMP_TEXTS), (stab, "DepanStabilise", STAB_ORDER, STAB_TEXTS)], ids=["compensate", "stabilise"])
def test_the_messages_in_the_integer_entries_order(mv, make, name, order, texts):
    for k in range(len(order)):
        with pytest.raises(mv.MvtoolsError) as got:
            make(mv, **dict(list(order.items())[k:]))
        assert str(got.value) == name + ": " + texts[k]
    # the same arguments through the integer entry, with a 32-bit clip: the reference's format message at that place
    for k in range(len(order)):
        with pytest.raises(mv.MvtoolsError) as got:
            make(mv, sample_float=False, **dict(dict(list(order.items())[k:]), bits=32))
        want = texts[k] if k < list(order).index("bits") else FORMAT    # bits=32 is wrong in every call of this loop
        assert str(got.value) == name + ": " + want


@pytest.mark.parametrize("make,name", [(comp, "DepanCompensate"), (stab, "DepanStabilise")], ids=["compensate", "stabilise"])
def test_a_clip_that_is_not_32_bit_and_the_subsampling(mv, make, name):
    for bits in (8, 10, 16, 31, 33, 64, 0, -32):
        with pytest.raises(mv.MvtoolsError) as got:
            make(mv, bits=bits)
        assert str(got.value) == name + ": " + NOT32
    for sub in ((0, 1), (2, 1), (1, 2)):
        with pytest.raises(mv.MvtoolsError) as got:
            make(mv, subsampling=sub)
        assert str(got.value) == name + ": " + FORMAT
    for bits in (32,):
        with pytest.raises(mv.MvtoolsError) as got:
            make(mv, bits=bits, sample_float=False)
        assert str(got.value) == name + ": " + FORMAT              # the integer entries keep the reference's message
    for fmt in (dict(), dict(subsampling=(1, 0)), dict(subsampling=(0, 0)), dict(gray=True)):
        make(mv, **fmt)


@pytest.mark.parametrize("make,name", [(comp, "DepanCompensate"), (stab, "DepanStabilise")], ids=["compensate", "stabilise"])
def test_pitches_hold_a_row_and_are_multiples_of_4(mv, make, name):
    for kw in (dict(src_pitch=[255, 128, 128]), dict(src_pitch=[256, 126, 128]), dict(dst_pitch=[256, 128, 130]), dict(dst_pitch=[258, 128, 128]), dict(src_pitch=[252, 128, 128]),
               dict(dst_pitch=[256, 124, 128]), dict(src_pitch=[-256, 128, 128])):
        with pytest.raises(mv.MvtoolsError) as got:
            make(mv, 64, 64, **kw)
        assert str(got.value) == name + ": " + PITCH, kw
    g = make(mv, 64, 64, src_pitch=[256, 128, 128], dst_pitch=[260, 132, 136])   # tight, and padded by one sample; U and V may differ
    assert g.pitch == [260, 132, 136]
    make(mv, 64, 64, gray=True, src_pitch=[256, 1, 2], dst_pitch=[256, 0, 0])       # a Gray clip's chroma pitches are not read
    for args, kw in (((3, 64), {}), ((64, 3), {}), ((1, 64), dict(gray=True)), ((32768, 64), {}), ((64, 32768), {})):
        with pytest.raises(mv.MvtoolsError) as got:
            make(mv, *args, **kw)
        assert str(got.value) == name + ": " + SIZE
    make(mv, 2, 2, gray=True)
    make(mv, 4, 4)
    # the earlier messages come first
    with pytest.raises(mv.MvtoolsError) as got:
        make(mv, 3, 64, bits=16, src_pitch=[1, 1, 1])
    assert str(got.value) == name + ": " + NOT32


def _fields(info):
    return {f: (list(getattr(info, f)) if hasattr(getattr(info, f), "__len__") else getattr(info, f)) for f, _ in info._fields_}


@pytest.mark.parametrize("fmt", [dict(), dict(subsampling=(1, 0)), dict(subsampling=(0, 0)), dict(gray=True)], ids=["420", "422", "444", "gray"])
def test_info_of_a_float_object(mv, fmt):
    """everything equals the 16-bit object's but bits (32), pixel_max (0) and border[] (0: the border value is 0.0f luma, 0.5f chroma)"""
    kw = dict(subpixel=1, mirror=9, blur=5, **fmt)
    for make in (comp, stab):
        f, i = _fields(make(mv, **kw).info), _fields(make(mv, bits=16, sample_float=False, **kw).info)
        assert f["bits"] == 32 and f["pixel_max"] == 0 and f["border"] == [0, 0, 0]
        assert i["bits"] == 16 and i["pixel_max"] == 65535 and i["border"][0] == 0
        for k in f:
            if k not in ("bits", "pixel_max", "border"):
                assert f[k] == i[k], k
        assert f["blur"] == ([5, 5, 5] if fmt.get("gray") or fmt.get("subsampling") == (0, 0) else [5, 2, 2])
    g = comp(mv, **fmt)
    sw = 0 if fmt.get("gray") else fmt.get("subsampling", (1, 1))[0]
    assert g.dtype == np.float32 and g.is_float
    assert g.pitch == [((max(W >> s, 1) * 4 + 255) // 256) * 256 for s in (0, sw, sw)]       # default pitches for 4-byte samples
    assert not comp(mv, bits=8, sample_float=False).is_float and comp(mv, bits=8, sample_float=False).dtype == np.uint8


def test_the_host_arithmetic_is_shared(mv):
    """map, transform, window and plan of a float object against the 16-bit object's, bit for bit"""
    import depan_stab_cases as sc
    f, i = comp(mv, offset=-1.5, pixaspect=1.1), comp(mv, bits=16, sample_float=False, offset=-1.5, pixaspect=1.1)
    for n in range(12):
        assert f.map(n) == i.map(n)
    m = sc.track(3, 5)
    a, b = f.transform(m[:2]), i.transform(m[:2])
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    kw = dict(num_frames=40, prev=2, next=2, method=1, cutoff=2.0)
    f, i = stab(mv, **kw), stab(mv, bits=16, sample_float=False, **kw)
    m = sc.track(40, 6, bad=(17,))
    assert all(np.array_equal(x, y) for x, y in zip(f.windows(), i.windows()))
    for n in (0, 5, 16, 18, 39):
        assert f.window(n) == i.window(n)
        w = f.window(n)
        assert bytes(f.plan(n, m[w[0]:w[1] + 1])) == bytes(i.plan(n, m[w[0]:w[1] + 1]))
