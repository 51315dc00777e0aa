"""The scenes of the DepanEstimate tests.  A scene is low-pass noise at the clip's full sample range; `cur` is cut from the same canvas as `prev`,
displaced by a planted whole-pixel pan (so the filter should return that pan), or from an unrelated canvas (a scene change), or with its left and
right halves panned apart (zoom).  Each case states what it claims: tests/test_depan_estimate_ref.py holds every case to its claim, with margins
that exceed the distance between a single-precision and a double-precision FFT a thousandfold (peak) or a hundredfold (thresholds), so that a third
FFT -- the library's -- must land on the same side of every decision.  A case that misses its claim is replaced, never excused.

The windows (winx x winy): the smallest; unequal axes both ways; 256 x 128; the longest transform on either axis; and both sides of every length
at which the kernels change path -- the transforms per workgroup are clamp(8192 / n, 1, 32), which changes between each two of n = 256, 512, 1024,
2048, 4096, 8192, on the row passes (n = winx) and on the column passes (n = winy) -- PATH_LENGTHS below.  The LDS held by a workgroup never exceeds
64 KiB, so capacity adds no further path."""
import functools

import numpy as np

import depan_estimate_ref as er

PATH_LENGTHS = (256, 512, 1024, 2048, 4096, 8192)
WINDOWS = [(8, 8), (32, 16), (16, 64), (256, 128), (8192, 8), (8, 8192)] + [(n, 8) for n in PATH_LENGTHS[1:-1]] + [(8, n) for n in PATH_LENGTHS[:-1]]


def canvas(h, w, bits, seed, smooth=1, power=6):
    """noise, box-filtered `smooth` times with a 3 x 3 kernel (wrapping), raised to `power` and stretched to the full range of `bits`"""
    g = np.random.default_rng(seed).random((h, w))
    for _ in range(smooth):
        g = sum(np.roll(np.roll(g, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)) / 9.0
    g = ((g - g.min()) / (g.max() - g.min())) ** power   # power 6: bright features on a dark ground: a mean well below the deviation, a trust well above 4
    return np.round(g * ((1 << bits) - 1)).astype(np.uint16 if bits > 8 else np.uint8)


class Case:
    def __init__(self, name, width, height, bits, claim, seed, pan=(0, 0), pan2=None, n=1, prop=None, smooth=1, power=6, **kw):
        self.name, self.width, self.height, self.bits, self.claim, self.seed, self.pan, self.pan2, self.n, self.prop, self.smooth, self.power = \
            name, width, height, bits, claim, seed, pan, pan2, n, prop, smooth, power
        self.kw = kw

    def __repr__(self):
        return self.name

    def ref(self):
        return er.Estimate(self.width, self.height, self.bits, **self.kw)

    @functools.lru_cache(maxsize=None)
    def frames(self):
        """prev, cur: full luma planes"""
        W, H, m = self.width, self.height, 16
        big = canvas(H + 2 * m, W + 2 * m, self.bits, self.seed, self.smooth, self.power)
        cut = lambda c, p: c[m + p[1]:m + p[1] + H, m + p[0]:m + p[0] + W]
        prev = cut(big, (0, 0))
        if self.claim == "scene_change":
            cur = cut(canvas(H + 2 * m, W + 2 * m, self.bits, self.seed + 1000, self.smooth, self.power), (0, 0))
        elif self.claim == "bad_zoom_scene":
            other = canvas(H + 2 * m, W + 2 * m, self.bits, self.seed + 1000, self.smooth, self.power)
            cur = np.concatenate([cut(big, self.pan)[:, :W // 2], cut(other, self.pan2)[:, W // 2:]], axis=1)
        elif self.pan2 is not None:
            cur = np.concatenate([cut(big, self.pan)[:, :W // 2], cut(big, self.pan2)[:, W // 2:]], axis=1)
        else:
            cur = cut(big, self.pan)
        return np.ascontiguousarray(prev), np.ascontiguousarray(cur)

    @functools.lru_cache(maxsize=None)
    def result(self, which):
        """the restatement with the double (64) or the single-precision (32) FFT"""
        prev, cur = self.frames()
        return self.ref().pair(prev, cur, self.n, er.FFT64 if which == 64 else er.FFT32, self.prop)


def _window_cases():
    out = []
    for k, (wx, wy) in enumerate(WINDOWS):
        for bits in (8, 16):
            # a frame a little larger than its window; a pan inside the default search area of winx / 4, winy / 4
            pan = (-max(1, min(wx // 4 - 1, 5) - k % 2), max(1, min(wy // 4 - 1, 3) - k % 2))
            out.append(Case("w%dx%d_%dbit" % (wx, wy, bits), wx + 6, wy + 4, bits, "pan", 100 + k, pan=pan, smooth=0 if wx * wy == 64 else 1, winx=wx, winy=wy))
    return out


CASES = _window_cases() + [
    Case("w64x32_10bit", 80, 40, 10, "pan", 201, pan=(7, -3), winx=64, winy=32),
    # wleft / wtop non-zero and odd (the plane's pitch is no multiple of the window either: see the GPU test)
    Case("w32x16_odd_origin", 75, 37, 8, "pan", 202, pan=(3, 2), winx=32, winy=16, wleft=13, wtop=7),
    Case("w64x16_odd_origin_16bit", 91, 29, 16, "pan", 203, pan=(-9, 1), winx=64, winy=16, wleft=21, wtop=5),
    # the automatic window of a 64 x 48 frame
    Case("auto_64x48", 64, 48, 8, "pan", 204, pan=(5, -4)),
    # search area smaller than the default, and dymax = 0
    Case("w64x64_dxmax3", 70, 70, 8, "pan", 205, pan=(2, -1), winx=64, winy=64, dxmax=3, dymax=1),
    Case("w64x16_dymax0", 70, 20, 8, "pan", 206, pan=(-6, 0), winx=64, winy=16, dymax=0),
    # scene changes: unrelated scenes, under the default limit and under a limit of 20
    Case("scene_change_256x128", 256, 128, 8, "scene_change", 301, winx=256, winy=128),
    Case("scene_change_128x256_16bit", 140, 260, 16, "scene_change", 302, winx=128, winy=256, trust=20.0),
    # frame 0 gives zeros whatever the pair
    Case("frame0", 64, 48, 8, "frame0", 204, pan=(5, -4), n=0),
    # fields: from tff and from the per-frame property; pixaspect
    Case("fields_tff1_n3", 80, 40, 8, "pan", 401, pan=(4, 2), winx=64, winy=32, fields=True, tff=1, n=3),
    Case("fields_tff0_n3", 80, 40, 8, "pan", 401, pan=(4, 2), winx=64, winy=32, fields=True, tff=0, n=3),
    Case("fields_prop_top", 80, 40, 8, "pan", 402, pan=(-3, -2), winx=64, winy=32, fields=True, prop=1, n=2),
    Case("fields_prop_bottom", 80, 40, 8, "pan", 402, pan=(-3, -2), winx=64, winy=32, fields=True, prop=0, n=2),
    Case("pixaspect", 80, 40, 16, "pan", 403, pan=(6, 4), winx=64, winy=32, pixaspect=1.0940),
    # zoom: two windows, the halves panned apart
    Case("zoom_good", 160, 40, 8, "zoom", 501, pan=(-1, 1), pan2=(3, 1), winx=128, winy=32, zoommax=1.2),
    Case("zoom_good_16bit_auto", 256, 64, 16, "zoom", 502, pan=(1, -2), pan2=(5, -2), zoommax=1.1),
    Case("zoom_too_large", 160, 40, 8, "bad_zoom", 503, pan=(-6, 0), pan2=(6, 0), winx=128, winy=32, zoommax=1.1),
    Case("zoom_one_window_changes_scene", 520, 130, 8, "bad_zoom_scene", 504, pan=(-2, 0), pan2=(2, 0), winx=512, winy=128, zoommax=1.2, trust=20.0),
]
BY_NAME = {c.name: c for c in CASES}

# stage 3 (MVDepan.cpp:1200-1212) at trust_limit 4: (num_frames, n, trusts of frames max(0, n - 1), n, min(n + 1, num_frames - 1), is the motion zeroed).
# Written down by hand: a frame is zeroed when its trust is under 2 * limit = 8 AND under half its neighbour's, the previous neighbour counting only
# from frame 1 on and the next only before the last frame; a value exactly on either threshold does not zero.
_below = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))
_above = lambda v: float(np.nextafter(np.float32(v), np.float32(1e9)))
STAGE3 = [
    (10, 5, (20.0, 7.0, 7.0), True),
    (10, 5, (7.0, 7.0, 20.0), True),
    (10, 5, (14.0, 7.0, 14.0), False),            # exactly half of either neighbour
    (10, 5, (_above(14.0), 7.0, 14.0), True),
    (10, 5, (14.0, 7.0, _above(14.0)), True),
    (10, 5, (100.0, 8.0, 100.0), False),          # exactly 2 * limit
    (10, 5, (100.0, _below(8.0), 100.0), True),
    (10, 5, (100.0, 50.0, 100.0), False),
    (10, 0, (100.0, 3.0, 3.0), False),            # the first frame has no previous one (the caller's clamp hands it another trust: not read)
    (10, 0, (3.0, 3.0, 100.0), True),
    (10, 9, (3.0, 3.0, 100.0), False),            # the last frame has no next one
    (10, 9, (100.0, 3.0, 3.0), True),
    (1, 0, (100.0, 3.0, 100.0), False),
]
