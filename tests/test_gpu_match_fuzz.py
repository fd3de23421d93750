"""A 5-second, fixed-seed slice of tools/fuzz_match.py (the features matcher against its NumPy model over the generator's classes and
random layouts) under -m gpu.  The long soak is kept as a JSON summary under profiles/."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_match_slice(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_match
    out = fuzz_match.run(5.0, 20261119, verbose=True)
    print(out["per_class"], out["cases"], "cases")
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert sorted(out["per_class"]) == sorted(fuzz_match.CLASSES) and all(v >= 1 for v in out["per_class"].values()), out["per_class"]
