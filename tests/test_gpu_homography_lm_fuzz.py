"""A 5-second, fixed-seed slice of tools/fuzz_homography.py --refine (isx_find_homography_lm against tests/helpers/homography_lm_np.py over
the generator's classes, random layouts and lm_max_iters of 1, 2 and 10) under -m gpu.  Fragile cases (model margin < 1e-9) are skipped and
counted; more than 1 % of them fails the run.  Three fixed cases of the `large` class (400 .. 9 000 correspondences) run on top of
those the slice draws in its turn: 1.0 s for the three (6 905, 6 860 and 2 116 correspondences); the slice itself drew 9 `large` cases among 69 in its 5 s.  The long soak is kept as a JSON summary under profiles/."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_homography_lm_slice(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_homography
    out = fuzz_homography.run(5.0, 20261202, verbose=True, refine=True)
    print(out["per_class"], out["cases"], "cases", out["skipped_fragile"], "fragile")
    assert out["refine"] and out["mismatches"] == 0, out["failing_seeds"]
    assert not out["too_many_fragile"], (out["skipped_fragile"], out["cases"])
    assert sorted(out["per_class"]) == sorted(fuzz_homography.CLASSES) and all(v >= 1 for v in out["per_class"].values()), out["per_class"]


def test_fuzz_homography_lm_large_cases(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_homography
    counts = []
    for s in (20261202001, 20261202002, 20261202003):
        c = fuzz_homography.case(s, "large")
        iters = fuzz_homography.lm_iters_of(s)
        want = fuzz_homography.expected(c, iters)
        assert want[0]["margin"] >= 1e-9, s
        assert fuzz_homography.run_case(c, want, iters) == [], s
        counts.append(c["pairs"][0][1])
    assert min(counts) > 300, counts
