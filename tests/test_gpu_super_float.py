"""GPU: the float Super (mvx_super_create_float) against the numpy restatement (tests/super_float_ref.py, anchored to the oracle by
tests/test_super_float_ref.py): every defined rectangle sample for sample, every byte outside them still the zero the caller wrote, three frames
per call.  Geometries are the smallest that reach every path of the level-0 kernel:

    A  70 x 54   4:2:0 chroma is 35 x 27: odd widths, the scalar tail of the 8-sample store
    B  140 x 38  the padded luma of 172 x 70 crosses a 128-column tile seam
    C  36 x 36   with Gray and pad 0: a plane narrower than one tile, no padding"""
import numpy as np
import pytest

import degrain_float_cases as fc
import pipeline as pl
import super_float_ref as sf

pytestmark = pytest.mark.gpu

SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "gray": (1, 1)}
SIZES = {"A": (70, 54), "B": (140, 38), "C": (36, 36)}
PEL_SHARP = [(1, 2), (2, 0), (2, 1), (2, 2), (4, 0), (4, 1), (4, 2)]
FMT_PAD = [("420", (16, 16)), ("422", (8, 4)), ("444", (16, 16)), ("gray", (0, 0)), ("420", (8, 4)), ("444", (0, 0)), ("gray", (16, 16)), ("422", (16, 16)), ("420", (0, 0))]


def _cases():
    out, i = [], 0
    for size in ("A", "B"):
        for ps in PEL_SHARP:
            for _ in range(2):
                fmt, pad = FMT_PAD[i % len(FMT_PAD)]
                i += 1
                out.append((size, fmt, ps[0], ps[1], pad, False))
    out += [("C", "gray", pel, sharp, (0, 0), False) for pel, sharp in PEL_SHARP]
    out += [("C", "420", 2, 2, (16, 16), False), ("C", "444", 4, 1, (8, 4), False)]
    out += [("A", "420", 2, 2, (16, 16), True), ("B", "422", 4, 1, (8, 4), True), ("A", "444", 2, 0, (0, 0), True)]  # luma -0.2 .. 1.3
    return out


CASES = _cases()
_clips = {}


def _clip(size, fmt, overshoot):
    key = (size, fmt, overshoot)
    if key not in _clips:
        w, h = SIZES[size]
        frames = pl.moving_clip(w, h, 16, 3, seed=5, noise=3, sub=SUB[fmt])
        if fmt == "gray":
            frames = [[f[0]] for f in frames]
        _clips[key] = fc.float_clip(frames, 16, seed=2, overshoot=overshoot)
    return _clips[key]


def _id(c):
    return "%s-%s-pel%d-sharp%d-pad%dx%d%s" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1], "-overshoot" if c[5] else "")


def check_frames(mv, sup, got, frames, skw):
    """got: device super frames of `frames` (float32 planes) -> asserts the defined rectangles and the zeros around them"""
    import torch
    torch.cuda.synchronize()
    for f, fr in enumerate(frames):
        want, defined = sf.frame(fr, **skw)
        for p in range(sup.nplanes):
            assert got[f][p].shape == (sup.info.plane_height[p], sup.pitch[p])
            g = got[f][p].cpu().numpy().view(np.float32)
            full, mask = np.zeros(g.shape, np.float32), np.zeros(g.shape, bool)
            full[:, :want[p].shape[1]], mask[:, :want[p].shape[1]] = want[p], defined[p]
            assert want[p].shape == (sup.info.plane_height[p], sup.info.plane_width[p])
            assert pl.first_diff(np.where(mask, g, 0), full) == "", "frame %d plane %d" % (f, p)
            assert not g.view(np.uint32)[~mask].any(), "frame %d plane %d: written outside the defined rectangles" % (f, p)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_defined_rectangles_are_the_restatements_and_nothing_else_is_written(mv, case):
    size, fmt, pel, sharp, pad, overshoot = case
    w, h = SIZES[size]
    frames = _clip(size, fmt, overshoot)
    if overshoot:
        assert float(frames[0][0].min()) < -0.05 and float(frames[0][0].max()) > 1.05
    if fmt != "gray":
        assert float(frames[0][1].min()) < -0.01  # chroma is centred on 0
    sup = mv.Super(w, h, 32, subsampling=SUB[fmt], gray=fmt == "gray", hpad=pad[0], vpad=pad[1], pel=pel, sharp=sharp, sample_float=True)
    got = sup.build([mv.frame_to_device(f) for f in frames])
    check_frames(mv, sup, got, frames, dict(sub=SUB[fmt], gray=fmt == "gray", hpad=pad[0], vpad=pad[1], pel=pel, sharp=sharp))


def test_a_second_build_into_the_same_frames_and_from_host(mv):
    """out= reuses frames (the averaged planes of pel 4 are rewritten, their last column / row stays 0); from_host uploads float planes"""
    w, h = SIZES["A"]
    frames = _clip("A", "420", False)
    sup = mv.Super(w, h, 32, pel=4, sharp=1, sample_float=True)
    src = [mv.frame_to_device(f) for f in frames]
    out = sup.build(src)
    sup.build(list(reversed(src)), out=out)
    skw = dict(pel=4, sharp=1)
    check_frames(mv, sup, out, list(reversed(frames)), skw)
    want, _ = sf.frame(frames[0], **skw)
    check_frames(mv, sup, [sup.from_host(want)], frames[:1], skw)
    with pytest.raises(mv.MvtoolsError, match="Finest: float super clips are not supported."):
        sup.finest(out[:1])
