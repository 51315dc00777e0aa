"""Stage 2 of the speculative search's 16x16 row passes takes a window of seven blocks in STRIP form when its blocks share one refinement centre and
in BLOCK form otherwise.  RUN form (mvx_analyse_spec.h: RUN) stands between the two: a window whose blocks end on two or three centres, in runs of
consecutive blocks, is evaluated as two or three strips side by side -- 9 or 10 column lanes per candidate, 7 or 6 candidates per pass.  The form
decides only which lane of which pass computes a table entry: the vector blobs must be the oracle's, byte for byte.

The clips are cut along luma columns into regions of different motion, so that a window of the finest level holds a chosen number of runs: two, with
the cut at every block position 1-6 of a window; three; four (block form); a cut on a window boundary (two strip windows); a run whose pattern leaves
its blocks' limits (block form).  Grids of one window, a window plus a block, two windows, a group, a group plus a block, two groups plus a block;
walked forwards and backwards (the meander reverses the runs of a window); 16-bit and 8-bit (one strip buffer); one wave per chain and teams; the
default search (Hex2 on the finest level, exhaustive above), search=3 and pel 1.  Every case first asserts on the CPU, from the oracle's own vectors,
that a window of the grid holds exactly the runs it is about.  The same file passes when the form is compiled out (-DMVX_SPEC_NORUN)."""
import ctypes as C
import functools

import numpy as np
import pytest

import pipeline as pl

pytestmark = pytest.mark.gpu

WIN = 7                                          # blocks of a window; windows start at the multiples of 7 of a block row (groups of 28, frames of 56)
MOTIONS = ((5, -2), (-3, 1), (4, 3), (-6, -1))  # px per frame of the regions, left to right
ROWS = 3                                         # the first block row is searched live; a middle and the last row are speculated


@pytest.fixture
def dbg(mv):
    """kernel-variant switches for one test (mvx_debug_option: selects among kernels that compute identical results); reset afterwards"""
    used = []

    def set_(name, value):
        mv.debug_option(name, value)
        used.append(name)
    yield set_
    for name in used:
        mv.debug_option(name, -1 if name == "team" else 1 if name == "spec" else 0)


def _region_clip(w, h, bits, cuts, motions):
    """region i (luma columns cuts[i - 1] .. cuts[i] - 1) moves by motions[i] per frame: the same texture and noise, cut along even luma columns (4:2:0)"""
    clips = [pl.moving_clip(w, h, bits, 3, seed=23, noise=4, motion=m) for m in motions[:len(cuts) + 1]]
    edges = [0] + list(cuts) + [w]
    out = []
    for f in range(3):
        planes = []
        for p in range(3):
            e = edges if p == 0 else [x // 2 for x in edges]
            planes.append(np.ascontiguousarray(np.concatenate([clips[i][f][p][:, e[i]:e[i + 1]] for i in range(len(e) - 1)], axis=1)))
        out.append(planes)
    return out


@functools.lru_cache(maxsize=4)
def _oracle_side(w, h, bits, meander, search, pel, cuts, motions, hpad=None):
    """frames, the oracle's blobs (backward, forward; with and without a reference) and analysis data: the same for every form of the launch"""
    import mvoracle as oracle
    frames = _region_clip(w, h, bits, cuts, motions)
    osup = oracle.Super(w, h, bits, pel=pel, hpad=hpad)
    osf = [osup.frame(f) for f in frames]
    want = []
    for isb in (1, 0):
        oan = oracle.Analyse(osup, isb=isb, blksize=16, overlap=8, meander=meander, search=search)
        want.append((oan.frame(osf[1], osf[2 if isb else 0]), oan.frame(osf[1], None)))
    return frames, want, oan.ad


def _cut_x(block):
    """the luma column of a cut after which `block` is the first block of the next region: block - 1 (columns 8 block - 8 .. 8 block + 7) keeps twelve
    columns of the region on the left, `block` (8 block .. 8 block + 15) twelve of the region on the right"""
    return 8 * block + 4


def _run_starts(vx, vy, row, f, e):
    """positions (1 ..) inside the window of blocks f .. e - 1 at which a maximal run of equal vectors starts, the first run apart"""
    return [m for m in range(1, e - f) if (vx[row, f + m], vy[row, f + m]) != (vx[row, f + m - 1], vy[row, f + m - 1])]


def _windows(want, ad):
    """(vx, vy, row, first block, end) of every window of every speculated block row of the finest level, for both directions"""
    for o_ref, _ in want:
        vx, vy, _sad = pl.blob_vectors(o_ref, ad, 0)
        for row in range(1, ad.nBlkY):  # (the first block row is searched live)
            for f in range(0, ad.nBlkX, WIN):
                yield vx, vy, row, f, min(f + WIN, ad.nBlkX)


def _pattern_inside(vx, ad, b):
    """the five columns of the pattern around block b's vector lie inside the block's horizontal limits (the window's test for strip and run form)"""
    xs, pel = 8 * b, ad.nPel
    lo, hi = -((xs + ad.nHPadding) * pel), (ad.nWidth + ad.nHPadding - xs - 16) * pel - 1  # (the reference's nDxMin and nDxMax - 1 of the finest level)
    return vx - 2 >= lo and vx + 2 <= hi


def _need_runs(window, starts):
    """a window that starts at block `window` holds exactly the runs that start at `starts`, each with the whole pattern inside its limits"""
    def check(want, ad):
        for vx, vy, row, f, e in _windows(want, ad):
            if f == window and _run_starts(vx, vy, row, f, e) == list(starts) and all(_pattern_inside(int(vx[row, b]), ad, b) for b in range(f, e)):
                return
        raise AssertionError("no speculated block row has, in the window at block %d, exactly the runs that start at %s: this case does not cover what it is about" % (window, list(starts)))
    return check


def _need_two_strip_windows(window):
    """the windows at blocks `window` - 7 and `window` are both uniform, with different vectors"""
    def check(want, ad):
        for vx, vy, row, f, e in _windows(want, ad):
            if f == window and not _run_starts(vx, vy, row, f, e) and not _run_starts(vx, vy, row, f - WIN, f) and (vx[row, f], vy[row, f]) != (vx[row, f - 1], vy[row, f - 1]):
                return
        raise AssertionError("no speculated block row has two uniform windows with different vectors on the two sides of block %d" % window)
    return check


def _need_runs_outside_limits(window, starts):
    """a window with exactly the runs at `starts` in which one block's pattern leaves its limits: two runs, and still block form"""
    def check(want, ad):
        for vx, vy, row, f, e in _windows(want, ad):
            if f == window and _run_starts(vx, vy, row, f, e) == list(starts) and not all(_pattern_inside(int(vx[row, b]), ad, b) for b in range(f, e)):
                return
        raise AssertionError("no speculated block row has, in the window at block %d, the runs at %s with a pattern outside a block's limits" % (window, list(starts)))
    return check


def _case(mv, dbg, bits, nblkx, meander, team, cut_blocks, precondition, search=None, pel=None, motions=MOTIONS, hpad=None):
    w, h = 8 * nblkx + 8, 8 * ROWS + 8
    cuts = tuple(_cut_x(b) for b in cut_blocks)
    frames, want, ad = _oracle_side(w, h, bits, meander, search, pel, cuts, motions, hpad)
    assert (ad.nBlkX, ad.nBlkY) == (nblkx, ROWS), "the clip does not have the block grid this case is about"
    precondition(want, ad)  # (on the CPU, from the oracle's own vectors, before the GPU is used)
    dbg("team", team)
    gsup = mv.Super(w, h, bits, pel=pel, hpad=hpad)
    gsf = gsup.build([mv.frame_to_device(f) for f in frames])
    info = (C.c_int * 5)()
    for isb, (o_ref, o_none) in zip((1, 0), want):
        gan = mv.Analyse(gsup, isb=isb, blksize=16, overlap=8, meander=meander, search=search)
        got = gan.run([(gsf[1], gsf[2 if isb else 0]), (gsf[1], None)])
        mv.lib().mvx_debug_last_launch(info)
        assert info[4] == (3 if team else 2), "not the speculative kernel in the form this case is meant to cover (%s)" % list(info)
        if team:
            assert info[1] == team, list(info)
        assert got[0].cpu().numpy().tobytes() == o_ref.tobytes(), "vectors differ from the oracle (isb=%d)" % isb
        assert got[1].cpu().numpy().tobytes() == o_none.tobytes(), "the default vectors of a job without a reference differ (isb=%d)" % isb


@pytest.mark.parametrize("team", [0, 2, 4])
@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_two_runs_cut_at_every_block(mv, dbg, m, bits, meander, team):
    """two regions: the second run starts at block m of the second window (a group of four windows and one block more)"""
    _case(mv, dbg, bits, 29, meander, team, (WIN + m,), _need_runs(WIN, [m]))


# (blocks per row, the window that holds the cut, the block of the window at which the second run starts)
GRIDS = [(7, 0, 6), (8, 0, 6), (14, 7, 5), (28, 21, 5), (29, 0, 3), (57, 49, 4)]  # (the windows under the clip's moving rectangle hold more runs)


@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("nblkx,window,m", GRIDS)
def test_two_runs_grids(mv, dbg, nblkx, window, m, bits, meander):
    """one window, a window plus one block, two windows, a group, a group plus a short window, two groups plus a short window"""
    _case(mv, dbg, bits, nblkx, meander, 0, (window + m,), _need_runs(window, [m]))


@pytest.mark.parametrize("team", [0, 2, 4])
@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("bits", [16, 8])
def test_three_runs(mv, dbg, bits, meander, team):
    """three regions inside the second window: runs of two, three and two blocks"""
    _case(mv, dbg, bits, 29, meander, team, (WIN + 2, WIN + 5), _need_runs(WIN, [2, 5]))


@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("bits", [16, 8])
def test_four_runs_take_block_form(mv, dbg, bits, meander):
    """four regions inside the second window: more runs than the form holds"""
    _case(mv, dbg, bits, 29, meander, 0, (WIN + 2, WIN + 4, WIN + 6), _need_runs(WIN, [2, 4, 6]))


@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("bits", [16, 8])
def test_cut_on_a_window_boundary(mv, dbg, bits, meander):
    """the second region starts with the second window: two strip-form windows, no runs"""
    _case(mv, dbg, bits, 29, meander, 0, (WIN,), _need_two_strip_windows(WIN))


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("cut_blocks,starts", [((WIN + 3,), [3]), ((WIN + 2, WIN + 5), [2, 5])])
@pytest.mark.parametrize("search,pel", [(3, None), (None, 1)])
def test_runs_exhaustive_and_pel1(mv, dbg, search, pel, cut_blocks, starts, bits):
    """search=3: 24 points on the finest level too, four run-form passes of seven or six; pel 1: one plane, whole-pel pattern offsets"""
    _case(mv, dbg, bits, 29, 1, 0, cut_blocks, _need_runs(WIN, starts), search=search, pel=pel)


@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("bits", [16, 8])
def test_run_outside_its_limits_takes_block_form(mv, dbg, bits, meander):
    """a padding of four samples and a first region that moves by all four: its vector is the first block's limit, the pattern around it leaves the
    limits of that block, and the first window -- two runs -- stays in block form"""
    _case(mv, dbg, bits, 29, meander, 0, (3,), _need_runs_outside_limits(0, [3]), motions=((4, -1), (-3, 1)), hpad=4)
