"""A 5-second, fixed-seed slice of tools/fuzz_polar_warp.py (the fisheye and stereographic projectors against their NumPy model over the
generator's classes, entries and layouts) under -m gpu.  The long soak is kept as a JSON summary under profiles/."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_polar_warp_slice(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_polar_warp
    out = fuzz_polar_warp.run(5.0, 20261020, verbose=True)
    print(out["per_class"], out["per_entry"], out["cases"], "cases")
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert sorted(out["per_class"]) == sorted(fuzz_polar_warp.CLASSES) and all(v >= 1 for v in out["per_class"].values()), out["per_class"]
