"""A 5-second slice of tools/fuzz_orb.py: isx_orb_find against tests/helpers/orb_np.py over the seeded classes (blobs, noise, identical
dots, squares, a flat image; 40 to 330 pixels a side; 1, 3 and 4 channels; 1 to 9 cells; 0 to 600 features; 1 to 8 levels; five scale
factors; host, device and strided mats; a caller's pattern), and one of its limits family (more than 1024 candidates a layer, up to 1024
layers, sides of 1 to 70).  Every case is compared, none skipped; 0 mismatches."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_orb as fz  # noqa: E402

pytestmark = pytest.mark.gpu


def test_fuzz_slice(gpu):
    out = fz.run(5.0, 20261021)
    print(out)
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert out["cases"] >= len(fz.CLASSES) and min(out["per_class"].values()) >= 1 and sum(out["per_class"].values()) == out["cases"]


def test_fuzz_slice_of_the_limits_family(gpu):
    """5 seconds of --family limits: 700 to 1920 features on one or two levels, strips under grids of up to 1024 layers, sides of 1 to 70"""
    out = fz.run(5.0, 20261021, family="limits")
    print(out)
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert out["cases"] >= len(fz.LIMIT_KINDS) and min(out["per_class"].values()) >= 1 and sum(out["per_class"].values()) == out["cases"]
