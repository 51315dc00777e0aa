"""CPU tests of tests/layouts.py: the carved planes come out at the pitch and base residue asked for, intact() sees a byte planted in each of
its four regions and nothing else, and the layout tables contain -- at the sizes tests/test_gpu_layouts.py uses -- the layouts that the
aligned, padded planes of the other GPU tests never produce: an odd pitch, a pitch of 2 mod 4, a super pitch of 16 mod 32, U and V of
different pitch."""
import numpy as np
import pytest

import layouts as lo

SIZES = [(206, 118), (208, 120), (270, 72)]  # the clip sizes of the GPU layout tests, 4:2:0


@pytest.mark.parametrize("fill", list(lo.FILLS) + [lo.NAN_FILL])
@pytest.mark.parametrize("rows,row_bytes,pitch,residue", [(59, 103, 103, 0), (59, 103, 104, 0), (118, 412, 414, 0), (5, 206, 512, 1), (5, 412, 768, 6),
                                                          (7, 824, 1040, 12), (3, 528, 544, 16), (1, 4096, 4096, 48)])
def test_carve_gives_the_pitch_and_residue_asked_for(rows, row_bytes, pitch, residue, fill):
    arena, view = lo.carve(rows, row_bytes, pitch, residue, fill, device="cpu")
    assert view.data_ptr() % 256 == residue and view.stride(0) == pitch and tuple(view.shape) == (rows, pitch)
    start = view.data_ptr() - arena.data_ptr()
    assert start >= 8 * pitch + 256 and arena.numel() - (start + rows * pitch) >= 8 * pitch + 256
    assert view.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr()
    assert lo.intact(arena, view, row_bytes, fill) == []
    if not isinstance(fill, int):  # the NaN pattern falls on whole float32 samples of a plane that starts at a multiple of 4
        if residue % 4 == 0 and pitch % 4 == 0:
            assert np.isnan(view.numpy().reshape(-1).view(np.float32)).all()
    else:
        assert int(view.min()) == int(view.max()) == fill


@pytest.mark.parametrize("fill", list(lo.FILLS) + [lo.NAN_FILL])
def test_intact_reports_each_region_and_nothing_else(fill):
    rows, row_bytes, pitch = 6, 103, 110
    plant = 0x11

    def damaged(index):
        arena, view = lo.carve(rows, row_bytes, pitch, 3, fill, device="cpu")
        start = view.data_ptr() - arena.data_ptr()
        arena[start + index] = plant
        return lo.intact(arena, view, row_bytes, fill)

    end = rows * pitch
    assert damaged(-1) == [(lo.REGIONS[0], -1, pitch - 1, plant)]
    assert damaged(-(8 * pitch + 200)) == [(lo.REGIONS[0], -10, (-(8 * pitch + 200)) % pitch, plant)]
    assert damaged(2 * pitch + row_bytes) == [(lo.REGIONS[1], 2, row_bytes, plant)]          # the first byte behind a row's samples
    assert damaged(end - 1) == [(lo.REGIONS[1], rows - 1, pitch - 1, plant)]                  # the last row's tail belongs to the plane
    assert damaged(end) == [(lo.REGIONS[2], rows, 0, plant)]
    assert damaged(end + 8 * pitch - 1) == [(lo.REGIONS[2], rows + 7, pitch - 1, plant)]
    assert damaged(end + 8 * pitch) == [(lo.REGIONS[3], rows + 8, 0, plant)]
    # samples are not guarded: writing them is the filter's job
    assert damaged(0) == [] and damaged(3 * pitch + row_bytes - 1) == []
    # all four at once, in order, and the message names row and column of the first
    arena, view = lo.carve(rows, row_bytes, pitch, 3, fill, device="cpu")
    start = view.data_ptr() - arena.data_ptr()
    for i in (-5, pitch + row_bytes + 2, end + 7, end + 8 * pitch + 9):
        arena[start + i] = plant
    got = lo.intact(arena, view, row_bytes, fill)
    assert [g[0] for g in got] == list(lo.REGIONS)
    assert lo.describe(got).startswith("before the plane: first damaged byte at row -1, column %d (now 0x11)" % (pitch - 5))


def test_a_tight_plane_has_no_row_tails():
    arena, view = lo.carve(4, 206, 206, 0, 0xA5, device="cpu")
    view[:] = 0
    assert lo.intact(arena, view, 206, 0xA5) == []
    arena[view.data_ptr() - arena.data_ptr() + 4 * 206] = 0  # one sample too many lands in the guard row
    assert lo.intact(arena, view, 206, 0xA5) == [(lo.REGIONS[2], 4, 0, 0)]


def test_put_and_get_round_trip():
    for dtype, bps in ((np.uint8, 1), (np.uint16, 2), (np.float32, 4)):
        a = (np.arange(59 * 103) % 251).astype(dtype).reshape(59, 103)
        pitch, residue = lo.clip_layout("offset3", 103, bps)
        arena, view = lo.carve(59, 103 * bps, pitch, residue, 0x5A, device="cpu")
        lo.put(view, a)
        assert np.array_equal(lo.get(view, 103, dtype), a)
        assert lo.intact(arena, view, 103 * bps, 0x5A) == []


def test_the_clip_layout_table_holds_the_layouts_the_aligned_tests_never_see():
    pitches = {}
    for (w, h) in SIZES:
        for bps in (1, 2, 4):
            for name in lo.CLIP_LAYOUTS:
                for plane, pw in enumerate((w, w // 2, w // 2)):
                    pitch, residue = lo.clip_layout(name, pw, bps, plane)
                    assert pitch >= pw * bps and pitch % bps == 0 and residue % bps == 0 and residue < 256, "every layout is legal"
                    pitches[(w, bps, name, plane)] = (pitch, residue)
    # the control is today's layout
    assert pitches[(206, 1, "padded", 0)] == (256, 0) and pitches[(206, 2, "padded", 1)] == (256, 0)
    # tight: pitch == row bytes; the 4:2:0 chroma of 206 is 103 wide: an odd pitch at 8 bit; 206 bytes are 2 mod 4
    assert pitches[(206, 1, "tight", 1)] == (103, 0) and pitches[(206, 1, "tight", 0)] == (206, 0)
    assert pitches[(206, 1, "tight", 1)][0] % 2 == 1 and pitches[(206, 1, "tight", 0)][0] % 4 == 2
    # plus1: odd for 8 bit, 2 mod 4 for 16 bit whenever the width is even
    assert pitches[(208, 1, "plus1", 0)] == (209, 0) and pitches[(208, 2, "plus1", 0)][0] % 4 == 2 and pitches[(270, 2, "plus1", 0)][0] % 4 == 2
    # offset: bases that are multiples of the sample size only
    assert pitches[(206, 1, "offset", 0)] == (512, 1) and pitches[(206, 1, "offset3", 0)] == (512, 3)
    assert pitches[(206, 2, "offset", 0)] == (768, 2) and pitches[(206, 2, "offset3", 0)] == (768, 6)
    # float planes: every pitch and residue a multiple of 4
    assert all(p % 4 == 0 and r % 4 == 0 for (w, bps, _, _), (p, r) in pitches.items() if bps == 4)
    assert pitches[(206, 4, "offset", 0)][1] == 4 and pitches[(206, 4, "offset3", 0)][1] == 12
    # U != V
    for (w, _h) in SIZES:
        for bps in (1, 2, 4):
            assert pitches[(w, bps, "uv_differ", 2)][0] == pitches[(w, bps, "uv_differ", 1)][0] + 256
            assert pitches[(w, bps, "uv_differ", 0)] == pitches[(w, bps, "padded", 0)]
    got = [p for p, _ in pitches.values()]
    assert any(p % 2 == 1 for p in got) and any(p % 4 == 2 for p in got)


def test_the_super_layout_table():
    for row in (206 + 32, 2 * (206 + 32), 103 + 16, 2 * (270 + 32), 4 * (206 + 32), 512):
        a, b = lo.super_pitch("sup16", row), lo.super_pitch("sup256", row)
        assert a >= row + 16 and a % 32 == 16, "an odd number of 16-byte units"
        assert a - lo.ceil_to(row, 16) in (16, 32)
        assert b == lo.ceil_to(row, 256) + 16 and b % 256 == 16
    for name in lo.SUPER_LAYOUTS:
        r = lo.super_residue(name)
        assert r % 16 == 0 and r % 256 != 0, "16-byte aligned, not 256-byte aligned"
