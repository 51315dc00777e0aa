"""Generates tests/golden/ref_objects.json: the results of the reference's own object code (oracle/_ref, which __graft_entry__.build()
compiles where the reference tree is present) on the inputs of the *_against_reference_object(s) tests of tests/test_oracle.py, in the
order those tests compare them: integers as they are, arrays as SHA-1 prefixes.  Without oracle/_ref the tests check the oracle against
this record.  Run from the repo root after build():  python tests/golden/make_ref_objects.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mvoracle  # noqa: E402
import test_oracle as t  # noqa: E402

if __name__ == "__main__":
    if not os.path.exists(t.REF_SO):
        sys.exit("oracle/_ref/libmvref.so is not built")
    mvoracle.lib()
    t._RECORDING = {}
    for test in (t.test_sad_satd_against_reference_objects, t.test_overlap_against_reference_objects, t.test_refine_kernels_against_reference_objects,
                 t.test_mask_upsizer_against_reference_object):
        test(mvoracle)
    with open(t.REF_RECORD, "w") as f:
        json.dump(dict(generator="tests/golden/make_ref_objects.py", **t._RECORDING), f, indent=0)
        f.write("\n")
    print({k: len(v) for k, v in t._RECORDING.items()})
