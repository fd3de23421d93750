"""A 5-second slice of tools/fuzz_estimator.py: isx_estimate_cameras against tests/helpers/estimator_np.py over the seeded classes (2, 3,
8, 9, 16, 17, 63 and 64 images in the first rig; one to five rigs; bare trees to complete graphs; tied weights; pairs without H; host, device
and strided mats; exactly singular H).  Every case is compared, none skipped; 0 mismatches."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_estimator as fz  # noqa: E402

pytestmark = pytest.mark.gpu


def test_fuzz_slice(gpu):
    out = fz.run(5.0, 20261020)
    print(out)
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert out["cases"] >= len(fz.CLASSES) and min(out["per_class"].values()) >= 1 and sum(out["per_class"].values()) == out["cases"]
