"""CPU companion of tests/test_gpu_small_geometry.py: what its cases are good for, shown on the oracle -- every case gives valid blobs (and a
default one where the reference lies outside the clip), the cases listed as having an empty legal rectangle have one and keep the zero vector
there, some case has non-zero vectors on every level, and the consumers run on the vectors of the unpadded clips."""
import numpy as np
import pytest

import pipeline as pl
import small_geometry_cases as sg
from test_gpu_small_geometry import CONSUMERS, NF, _ref

EMPTY_NAMES = {g["name"] for g in sg.EMPTY}


@pytest.fixture(scope="module")
def searched(oracle):
    """name -> (analysis data, [variant][frame] blobs) of every GPU search case, through the oracle"""
    out = {}
    for g in sg.GPU_SEARCHES:
        frames = sg.clip(g, NF)
        osup, _ = sg.make(oracle, g, NF)
        osf = [osup.frame(f) for f in frames]
        per = []
        for v in sg.VARIANTS:
            if g["fmt"] == "gray" and "chroma" in v:
                continue
            _, oan = sg.make(oracle, g, NF, **v)
            per.append((v, oan.ad, [oan.frame(osf[n], osf[_ref(v, n)] if _ref(v, n) is not None else None) for n in range(NF)]))
        out[g["name"]] = per
    return out


def test_every_case_has_valid_blobs_and_default_ones_at_the_clip_ends(searched):
    for name, per in searched.items():
        for v, ad, blobs in per:
            for n, b in enumerate(blobs):
                hdr = b[:8].view(np.int32)
                assert hdr[0] == len(b) and hdr[1] == (1 if _ref(v, n) is not None else 0), (name, v, n, list(hdr))
            assert any(_ref(v, n) is None for n in range(NF)) and any(_ref(v, n) is not None for n in range(NF))


def test_gpu_cases_hold_the_case_that_faulted_and_empty_rectangles(mv, searched):
    """the library's own level table: a level where nDxMax <= nDxMin and nDyMax <= nDyMin for some block (PlaneOfBlocks.cpp:1094-1097)"""
    names = [g["name"] for g in sg.GPU_SEARCHES]
    assert names[0] == sg.FAULTING["name"] and sg.SINGLE_BLOCK["name"] not in names
    have = 0
    for g in sg.GPU_SEARCHES:
        _, an = sg.make(mv, g)
        step = g["akw"]["blksize"] - g["akw"]["overlap"]
        empty = []
        for lvl, L in enumerate(an.levels()):
            nbx, nby, pel, pw, ph, hpad, vpad = L[:7]
            x0, y0 = hpad + step * (nbx - 1), vpad + step * (nby - 1)
            ex = (pw - x0 - g["akw"]["blksize"] - hpad + (hpad >> lvl)) * pel <= -((x0 - hpad + (hpad >> lvl)) * pel)
            ey = (ph - y0 - g["akw"]["blksize"] - vpad + (vpad >> lvl)) * pel <= -((y0 - vpad + (vpad >> lvl)) * pel)
            if ex and ey:
                empty.append(lvl)
        if g["name"] in EMPTY_NAMES:
            assert empty == [len(an.levels()) - 1], (g["name"], empty)
            have += 1
            # ... where the oracle evaluates the clipped predictors and keeps the zero vector
            for v, ad, blobs in searched[g["name"]]:
                x, y, _ = pl.blob_vectors(blobs[1], ad, level=empty[0])
                assert not x.any() and not y.any()
    assert have >= 5


def test_some_case_moves_on_every_level(searched):
    moving = []
    for name, per in searched.items():
        v, ad, blobs = per[0]
        if ad.nLvCount >= 2 and all(pl.blob_vectors(blobs[1], ad, level=l)[0].any() or pl.blob_vectors(blobs[1], ad, level=l)[1].any() for l in range(ad.nLvCount)):
            moving.append(name)
    assert moving, "no case has a non-zero vector on every level"


@pytest.mark.parametrize("g", CONSUMERS, ids=[g["name"] for g in CONSUMERS])
def test_consumers_run_on_these_vectors(oracle, g):
    frames = sg.clip(g, NF)
    osup, _ = sg.make(oracle, g, NF)
    osf = [osup.frame(f) for f in frames]
    blobs, refs = [], []
    for isb in (1, 0):
        _, oan = sg.make(oracle, g, NF, isb=isb)
        r = 2 + (1 if isb else -1)
        blobs.append(oan.frame(osf[2], osf[r]))
        refs.append(osf[r])
        rc = oracle.Recalculate(osup, oan.ad, blksize=4, overlap=2, thsad=60).frame(osf[2], osf[r], blobs[-1])
        assert rc[:8].view(np.int32)[1] == 1
    out = oracle.Degrain(1, osup, oan.ad).frame(frames[2], refs, blobs)
    assert any(not np.array_equal(out[p], frames[2][p]) for p in range(len(out)))  # it denoised something
