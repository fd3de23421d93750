"""A 5-second, fixed-seed slice of tools/fuzz_sift.py (the SIFT finder against its NumPy model over the generator's classes and random
layouts) under -m gpu.  A longer soak is a command in DESIGN.md §8, not a test."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_sift_slice(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_sift
    out = fuzz_sift.run(5.0, 20261221, verbose=True)
    print(out["per_class"], out["cases"], "cases")
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert all(out["per_class"][c] >= 1 for c in fuzz_sift.CLASSES), out["per_class"]
