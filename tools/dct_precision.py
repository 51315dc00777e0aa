"""What the float32 arithmetic of the dct 1..4 cost modes (csrc/mvx_dct_block.h) costs against float64, on the CPU -- no GPU involved: the device is held
byte for byte to the host build of the same text by the test suite.

    python tools/dct_precision.py

1. Per block shape and bit depth, on the seeded blocks of tests/dct_ref.py: the share of quantised coefficients the proven bound leaves undetermined
   (8 and 10 bits) and the share that differs from the float64 byte (12 to 16 bits), for the library's arithmetic and for scipy's single-precision dctn.
2. Report only: the share of blocks whose vector differs between the CPU oracle driven by the library's arithmetic and the same oracle driven by a
   float64 DCT, on two clips.  A cost that moves by one legitimately flips ties, so this says how often, not whether anything is wrong."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import dct_oracle as do  # noqa: E402
import dct_ref as dr  # noqa: E402
import pipeline as pl  # noqa: E402


def shares():
    for bits in (8, 10, 12, 14, 16):
        for bw, bh in dr.SHAPES:
            blocks, shift = dr.make_blocks(bw, bh, bits), dr.dct_shift(bw, bh)
            undet = total = diff = sdiff = 0
            worst = 0.0
            for b in blocks:
                y64, E = dr.coeffs64(b), dr.error_bound(b)
                ref = dr.quantise(y64, bits, shift)
                undet += int((~dr.determined(y64, E, bits, shift)).sum())
                total += ref.size
                diff += int((do.emu_bytes(b, bits).astype(np.int64) != ref).sum())
                sdiff += int((dr.quantise(dr.coeffs32_scipy(b), bits, shift) != ref).sum())
                if E > 0:
                    worst = max(worst, float(np.abs(do.emu_coeffs(b, bits).astype(np.float64) - y64).max()) / E)
            print("%2d-bit %2dx%-2d  undetermined by E %7.4f %%   largest error %.3f E   differs from float64: library %.2e  scipy float32 %.2e" % (
                bits, bw, bh, 100.0 * undet / total, worst, diff / total, sdiff / total), flush=True)


def vectors():
    o32, o64 = do.module(False), do.module(True)
    for name, w, h, bits, akw, ramp in (("128x80 8-bit, blksize 8 overlap 4, dct=1", 128, 80, 8, dict(blksize=8, overlap=4, dct=1), 0),
                                        ("256x144 16-bit, blksize 16 overlap 8, dct=4, brightness ramp", 256, 144, 16, dict(blksize=16, overlap=8, dct=4), 40)):
        frames = pl.moving_clip(w, h, bits, 3, seed=11, noise=3)
        if ramp:
            do.luma_ramp(frames, bits, ramp)
        blobs = []
        for o in (o32, o64):
            sup = o.Super(w, h, bits)
            sf = [sup.frame(f) for f in frames]
            an = o.Analyse(sup, **akw)
            blobs.append(([an.frame(sf[0], sf[1]), an.frame(sf[1], sf[0]), an.frame(sf[1], sf[2])], an.ad))
        moved = sads = n = 0
        for a, b in zip(blobs[0][0], blobs[1][0]):
            ax, ay, asad = pl.blob_vectors(a, blobs[0][1], 0)
            bx, by, bsad = pl.blob_vectors(b, blobs[0][1], 0)
            moved += int(((ax != bx) | (ay != by)).sum())
            sads += int((asad != bsad).sum())
            n += ax.size
        print("%s: %d of %d finest-level blocks take another vector (%.3f %%), %d another sad (%.3f %%)" % (name, moved, n, 100.0 * moved / n, sads, 100.0 * sads / n), flush=True)


if __name__ == "__main__":
    shares()
    vectors()
