"""Writes tests/golden/mask_ref_objects.json: digests of the reference's AVX2 uint8 mask resizer (SimpleResize_AVX2.cpp, from oracle/_ref)
on mv.Mask's unpadded geometries that tests/test_mask_host.py uses, so that the test also runs where oracle/_ref is absent.

    python tests/golden/make_mask_ref_objects.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"),
                os.path.join(os.path.dirname(os.path.dirname(HERE)), "vapoursynth-mvtools_amd")]

import test_flow_ref as t  # noqa: E402
import test_mask_host as m  # noqa: E402

if __name__ == "__main__":
    lib = t.ref_lib()
    assert lib is not None, "needs oracle/_ref (make -C oracle ref)"
    out = [t.digest(m.ref_resize_u8(lib, *g)) for g in m.GEOMETRIES]
    with open(os.path.join(HERE, "mask_ref_objects.json"), "w") as f:
        json.dump({"simpleResize_uint8_t_avx2": out}, f, indent=1)
    print("wrote %d digests" % len(out))
