"""CPU tests of the arithmetic of the dct 1..4 cost modes: csrc/mvx_dct_block.h compiled for the host (tests/dct_emu.cpp) against the float64
yardstick tests/dct_ref.py -- the proven error bound at 8 and 10 bits, the measured tolerance at 12, 14 and 16 bits, and the cost formulas
(DESIGN.md 4.2.9)."""
import numpy as np
import pytest

import dct_oracle as do
import dct_ref as dr

_cache = {}


def _case(bw, bh, bits):
    """blocks, exact coefficients, emu coefficients, emu bytes, float64 bytes of one (shape, depth): computed once, shared, never modified"""
    key = (bw, bh, bits)
    if key not in _cache:
        blocks = dr.make_blocks(bw, bh, bits)
        shift = dr.dct_shift(bw, bh)
        y64 = [dr.coeffs64(b) for b in blocks]
        _cache[key] = dict(blocks=blocks, shift=shift, y64=y64, y32=[do.emu_coeffs(b, bits) for b in blocks],
                           emu=[do.emu_bytes(b, bits).astype(np.int64) for b in blocks], ref=[dr.quantise(y, bits, shift) for y in y64])
    return _cache[key]


def test_generator_and_shift():
    assert [dr.dct_shift(*s) for s in dr.SHAPES] == [4, 6, 8, 10, 5, 5]
    b = dr.make_blocks(8, 4, 10)
    assert len(b) == 403 and b[0].shape == (4, 8) and b[0].dtype == np.uint16 and int(b[401].min()) == 1023 and int(b[400].max()) == 0
    assert all(np.array_equal(x, y) for x, y in zip(b, dr.make_blocks(8, 4, 10)))


def test_emu_quantiser_is_the_reference_s():
    """the quantiser of mvx_dct_block.h against the numpy statement of Float2Pixels_C, on values around every rounding and clamping edge"""
    L = do.emu()
    rng = np.random.default_rng(3)
    for bits, shift in ((8, 4), (8, 10), (10, 6), (16, 8), (16, 10)):
        vals = np.concatenate([rng.uniform(-3e8, 3e8, 2000), rng.uniform(-5000, 5000, 2000), (np.arange(-40, 40) + 0.5) / float(dr.SQRT_2_DIV_2),
                               np.arange(-41, 41, dtype=np.float64)]).astype(np.float32)
        for dc in (0, 1):
            for v in vals:
                g = np.float32(v) * (np.float32(0.5) if dc else dr.SQRT_2_DIV_2)
                want = min(max((int(np.rint(g)) >> (shift + 2 if dc else shift)) + (1 << (bits - 1)), 0), (1 << bits) - 1)
                assert L.dct_emu_quant(float(v), dc, shift, bits) == want, (bits, shift, dc, float(v))


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("bw,bh", dr.SHAPES)
def test_exact_bound(bw, bh, bits):
    """Every byte the proven bound E determines equals the float64 byte; at most 2 % are undetermined; the observed error stays below E."""
    c = _case(bw, bh, bits)
    total = undet = 0
    worst = 0.0
    for blk, y64, y32, emu, ref in zip(c["blocks"], c["y64"], c["y32"], c["emu"], c["ref"]):
        E = dr.error_bound(blk)
        err = float(np.abs(y32.astype(np.float64) - y64).max())
        assert err <= E, (err, E)
        if E > 0:
            worst = max(worst, err / E)
        det = dr.determined(y64, E, bits, c["shift"])
        assert np.array_equal(emu[det], ref[det]), "a determined byte differs from the float64 byte"
        total += det.size
        undet += int((~det).sum())
    print("dct %dx%d %d-bit: undetermined %.4f %%, largest error %.3f E" % (bw, bh, bits, 100.0 * undet / total, worst))
    assert undet <= 0.02 * total


@pytest.mark.parametrize("bits", [12, 14, 16])
@pytest.mark.parametrize("bw,bh", dr.SHAPES)
def test_measured_tolerance(bw, bh, bits):
    """Where the proven bound says little: every byte that differs from the float64 byte differs by exactly 1, and at most 1e-3 of them do."""
    c = _case(bw, bh, bits)
    emu, ref = np.stack(c["emu"]), np.stack(c["ref"])
    d = np.abs(emu - ref)
    assert int(d.max()) <= 1
    sc = np.stack([dr.quantise(dr.coeffs32_scipy(b), bits, c["shift"]) for b in c["blocks"]])
    print("dct %dx%d %d-bit: emu differs from float64 in %.2e of the bytes, scipy's float32 dctn in %.2e" % (
        bw, bh, bits, float((d != 0).mean()), float((sc != ref).mean())))
    assert float((d != 0).mean()) <= 1e-3


def test_cost_formula_on_a_grid():
    L = do.emu()
    rng = np.random.default_rng(5)
    for _ in range(4000):
        mode, bw = int(rng.integers(1, 5)), int(rng.choice([4, 8, 16, 32]))
        sad, ds, dc = int(rng.integers(0, 1 << 26)), int(rng.integers(0, 1 << 26)), int(rng.integers(0, 1 << 16))
        hit, w = int(rng.integers(0, 2)), int(rng.choice([0, 1, 8, 15, 16]))
        assert L.dct_emu_cost_formula(mode, sad, ds, dc, bw, hit, w) == dr.cost(mode, sad, ds, dc, bw, bool(hit), w)
    # the largest legal operands (32x32 at 16 bits) stay exact in 64 bits
    big = 1024 * 65535
    assert L.dct_emu_cost_formula(1, big, big, 65535, 32, 0, 0) == (big + 3 * 65535) * 16


def _threshold_lumas(ref_luma):
    """source luma sums exactly on (no switch) and one past (switch) the >> 5 threshold of modes 3 / 4, above the reference's"""
    s = ref_luma
    while not dr.luma_hit(s, ref_luma):
        s += 1
    assert dr.luma_hit(s, ref_luma) and not dr.luma_hit(s - 1, ref_luma)
    return s - 1, s


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("bw,bh", dr.SHAPES)
def test_costs_on_determined_blocks(bw, bh, bits):
    """the whole luma cost, emu against the float64 yardstick, on pairs of blocks whose bytes are all determined: modes 1..4, dctweight16 0 / 8 / 16,
    luma sums exactly on and one past the threshold"""
    c = _case(bw, bh, bits)
    good = [i for i, (blk, y64) in enumerate(zip(c["blocks"], c["y64"])) if dr.determined(y64, dr.error_bound(blk), bits, c["shift"]).all()]
    if bw * bh < 1024:
        assert len(good) >= 20, "too few fully determined blocks: %d" % len(good)
    pairs = list(zip(good[0::2], good[1::2]))[:12]
    for i, j in pairs:
        src, ref = c["blocks"][i], c["blocks"][j]
        on, past = _threshold_lumas(int(ref.astype(np.int64).sum()))
        for mode, luma, w in [(1, 0, 0), (2, 0, 0), (2, 0, 8), (2, 0, 16), (3, on, 0), (3, past, 0), (4, on, 0), (4, past, 0)]:
            want = dr.luma_cost(src, ref, bits, mode, luma, w)
            assert do.emu_luma_cost(src, ref, bits, mode, luma, w) == want, (mode, luma, w)
        sad = int(np.abs(src.astype(np.int64) - ref.astype(np.int64)).sum())
        assert do.emu_luma_cost(src, ref, bits, 3, on, 0) == sad and do.emu_luma_cost(src, ref, bits, 2, 0, 0) == sad
