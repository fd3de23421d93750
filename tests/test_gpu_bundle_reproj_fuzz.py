"""A 5-second slice of tools/fuzz_bundle_reproj.py: isx_bundle_adjust_reproj against tests/helpers/bundle_reproj_np.py over the seeded classes
of tools/fuzz_bundle.py with planted ppx / ppy / aspect offsets and random refine_flags on top, every fourth case a rig that goes round.  Every case is compared, none skipped; 0
mismatches."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_bundle_reproj as fz  # noqa: E402

pytestmark = pytest.mark.gpu


def test_fuzz_slice(gpu):
    out = fz.run(5.0, 20261203)
    print(out)
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert out["cases"] >= len(fz.CLASSES) and min(out["per_class"].values()) >= 1 and sum(out["per_class"].values()) + out["wide"] == out["cases"]
    assert out["wide"] >= 1 and out["wide"] == sum(out["per_wide_class"].values())          # every fourth case is a rig that goes round
