"""A 5-second, fixed-seed slice of tools/fuzz_match_f32.py (the float features matcher against its NumPy model over the generator's classes
and random layouts) under -m gpu, and one fixed case of the `split` class on top of those the slice draws in its turn.  The long soak is
kept as a JSON summary under profiles/."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_match_f32_slice(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_match_f32
    out = fuzz_match_f32.run(5.0, 20261121, verbose=True, with_split=False)
    print(out["per_class"], out["cases"], "cases")
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert all(out["per_class"][c] >= 1 for c in fuzz_match_f32.CLASSES[:-1]), out["per_class"]
    c = fuzz_match_f32.case(20261121004, "split")
    assert max(d.shape[0] for d in c["descriptors"]) >= 8191 and fuzz_match_f32.run_case(c) == []
