"""A 5-second, fixed-seed slice of tools/fuzz_surf.py (the SURF finder against its NumPy model over the generator's classes and random
layouts) under -m gpu.  The long soak is kept as a JSON summary under profiles/."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_surf_slice(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_surf
    out = fuzz_surf.run(5.0, 20261201, verbose=True)
    print(out["per_class"], out["cases"], "cases")
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert all(out["per_class"][c] >= 1 for c in fuzz_surf.CLASSES), out["per_class"]
