"""Float64 yardstick of the dct 1..4 cost modes: scipy's DCT-II in double precision, the reference's quantiser (DCTFFTW.cpp:30-54) and the four
cost formulas of pobLumaSAD (PlaneOfBlocks.cpp:123-163) in numpy, and the generator of the test blocks.  It bounds the precision of the
library's float32 arithmetic (csrc/mvx_dct_block.h); it is not what the library is held to byte for byte -- tests/dct_emu.cpp is."""
import numpy as np
import scipy.fft

SQRT_2_DIV_2 = np.float32(0.70710678118654752440084436210485)
SHAPES = [(4, 4), (8, 8), (16, 16), (32, 32), (8, 4), (16, 2)]  # (blksize, blksizev)


def dct_shift(bw, bh):
    shift, cur = 0, 1
    while cur < bw * bh:
        shift, cur = shift + 1, cur << 1
    return shift


def coeffs64(block):
    """fftw's REDFT10 x REDFT10: the unnormalised 2-D DCT-II, Y = 4 sum sum s cos cos (scipy's type 2 without `norm` is 2 sum s cos per axis)"""
    return scipy.fft.dctn(np.asarray(block, dtype=np.float64), type=2)


def coeffs32_scipy(block):
    """scipy's own single-precision transform: the stand-in for fftw3f"""
    return scipy.fft.dctn(np.asarray(block, dtype=np.float32), type=2)


def quantise(Y, bits, shift):
    """Float2Pixels_C on an array of coefficients (any float type; the product with sqrt(2)/2 is formed in float32 as the reference does after its
    float32 transform, in float64 for the float64 yardstick)"""
    Y = np.asarray(Y)
    half, mx = 1 << (bits - 1), (1 << bits) - 1
    k = SQRT_2_DIV_2 if Y.dtype == np.float32 else float(SQRT_2_DIV_2)
    q = (np.rint(Y * k).astype(np.int64) >> shift) + half
    q = np.clip(q, 0, mx)
    dc = (np.rint(Y.reshape(-1)[0] * (np.float32(0.5) if Y.dtype == np.float32 else 0.5)).astype(np.int64) >> (shift + 2)) + half
    q.reshape(-1)[0] = min(max(int(dc), 0), mx)
    return q


def quantise_scalar(v, dc, bits, shift):
    """the quantiser on one exact (float64) value: monotone in v"""
    half, mx = 1 << (bits - 1), (1 << bits) - 1
    g = v * (0.5 if dc else float(SQRT_2_DIV_2))
    return int(min(max((int(np.rint(g)) >> (shift + 2 if dc else shift)) + half, 0), mx))


def block_bytes64(block, bits):
    bh, bw = np.asarray(block).shape
    return quantise(coeffs64(block), bits, dct_shift(bw, bh))


def luma_hit(src_luma, ref_luma):
    return abs(src_luma - ref_luma) > ((src_luma + ref_luma) >> 5)


def cost(mode, sad, dct_sad, dc_abs, bw, hit, weight16):
    """pobLumaSAD for dct 1..4 on integers (C division of non-negative values == //)"""
    with_dc = (dct_sad + 3 * dc_abs) * bw // 2
    plain = dct_sad * bw // 2
    if mode == 1:
        return with_dc
    if mode == 2:
        return (sad * (16 - weight16) + with_dc * weight16) // 16 if weight16 > 0 else sad
    if mode == 3:
        return sad // 2 + plain // 2 if hit else sad
    if mode == 4:
        return sad // 4 + plain // 2 + plain // 4 if hit else sad
    return sad


def luma_cost(src, ref, bits, mode, src_luma, weight16, bytes_of=block_bytes64):
    """the whole luma term of one candidate from the two blocks"""
    src, ref = np.asarray(src, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    sad = int(np.abs(src - ref).sum())
    hit = mode in (3, 4) and luma_hit(int(src_luma), int(ref.sum()))
    a, b = bytes_of(src, bits), bytes_of(ref, bits)
    d = np.abs(a - b)
    return cost(mode, sad, int(d.sum()), int(d.reshape(-1)[0]), src.shape[1], hit, weight16)


def error_bound(block, c=6):
    """E: proven bound on |float32 transform - exact transform| of any coefficient of this block, DESIGN.md 4.2.9:
    (bw + bh + c) * 2^-24 * 4 * sum |s|"""
    bh, bw = np.asarray(block).shape
    return (bw + bh + c) * 2.0 ** -24 * 4.0 * float(np.abs(np.asarray(block, dtype=np.float64)).sum())


def quantise_exact(V, bits, shift):
    """quantise_scalar on a whole array of exact values (element 0 is the DC term)"""
    V = np.asarray(V, dtype=np.float64)
    half, mx = 1 << (bits - 1), (1 << bits) - 1
    q = (np.rint(V * float(SQRT_2_DIV_2)).astype(np.int64) >> shift) + half
    q.reshape(-1)[0] = (int(np.rint(V.reshape(-1)[0] * 0.5)) >> (shift + 2)) + half
    return np.clip(q, 0, mx)


def determined(Y64, E, bits, shift):
    """mask of the coefficients whose byte is the same for every value within E of the exact one (the quantiser is monotone)"""
    Y64 = np.asarray(Y64, dtype=np.float64)
    return quantise_exact(Y64 - E, bits, shift) == quantise_exact(Y64 + E, bits, shift)


def make_blocks(bw, bh, bits, n=400, seed=1):
    """n seeded blocks: a flat level plus Gaussian noise of sigma = max / 16, a quarter of them uniform noise; then all-0, all-max and a checker"""
    rng = np.random.default_rng(seed * 1000003 + bw * 131 + bh * 17 + bits)
    mx = (1 << bits) - 1
    out = []
    for i in range(n):
        if i % 4 == 3:
            b = rng.integers(0, mx + 1, (bh, bw))
        else:
            b = np.rint(rng.uniform(0, mx) + rng.normal(0, mx / 16.0, (bh, bw)))
        out.append(np.clip(b, 0, mx).astype(np.int64))
    yy, xx = np.mgrid[0:bh, 0:bw]
    out += [np.zeros((bh, bw), np.int64), np.full((bh, bw), mx, np.int64), ((xx + yy) & 1) * mx]
    dt = np.uint8 if bits <= 8 else np.uint16
    return [b.astype(dt) for b in out]
