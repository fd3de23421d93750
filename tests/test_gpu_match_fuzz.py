"""A 5-second, fixed-seed slice of tools/fuzz_match.py (the features matcher against its NumPy model over the generator's classes and
random layouts) under -m gpu, and four fixed cases of the `split` class (a train image past 8 192 rows) on top of those the slice draws in
its turn: 0.3 s for the four; the slice itself drew 33 cases of each of the seven classes in its 5 s.  The long soak is kept as a JSON summary under profiles/."""
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


def test_fuzz_match_split_cases(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_match
    shapes = set()
    for seed in (20261119003, 20261119004, 20261119005, 20261119006):      # 8193 x 129, 161 x 8192, 24576 x 116, 51 x 16385 rows
        c = fuzz_match.case(seed, "split")
        shapes.add(tuple(d.shape[0] for d in c["descriptors"]))
        assert fuzz_match.run_case(c) == [], seed
    assert len(shapes) == 4 and {s[0] > s[1] for s in shapes} == {True, False}, shapes
