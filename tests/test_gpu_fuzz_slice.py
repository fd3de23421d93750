"""A 20-second, fixed-seed slice of tools/fuzz_parity.py (the randomised HIP-vs-oracle sweep over every entry point, 28 families: warps, the
fused tile kernel, the blenders in all precisions and cycles, mask preparation, the seam finder, the linear pair blend, whole pairs through
PairStitcher, and - against their NumPy models - the plane projector, GainCompensator::feed, the Voronoi and graph-cut seam finders and
the COLOR_GRAD cost with seam_gradients, BlocksGainCompensator, cv::resize with the scaled mask stage, and the planned warp's ROI verification) under -m gpu, then 8 seconds of
the five families before the last three alone, whose shape classes sit on their kernels' tiling constants, 4 seconds of BlocksGainCompensator's,
4 seconds of cv::resize's, 4 seconds of GraphCutSeamFinder(COST_COLOR_GRAD)'s and 4 seconds of the last, the ROI verification's.  The long soaks are kept as JSON summaries under
profiles/."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_slice_20s(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_parity
    out = fuzz_parity.run(20.0, 20260928, verbose=True)
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert out["cases"] >= 100 and all(v["cases"] > 0 for v in out["per_family"].values()), out["per_family"]


def test_fuzz_slice_new_families(gpu):
    """The five families of the entry points merged after round 6, alone: each gets enough of the 8 seconds to run at least 5 cases."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_parity
    out = fuzz_parity.run(8.0, 20261017, verbose=True, only=fuzz_parity.NEW_FAMILIES)
    print(out["per_family"], "skipped", out["skipped_geometries"])
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert sorted(out["per_family"]) == sorted(fuzz_parity.NEW_FAMILIES)
    assert all(v["cases"] >= 5 for v in out["per_family"].values()), out["per_family"]
    assert out["skipped_geometries"] * 10 <= out["cases"], (out["skipped_geometries"], out["cases"])


def test_fuzz_slice_blocks_gain(gpu):
    """BlocksGainCompensator's family alone: feed (statistics, gains, maps) and apply over its seven shape classes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_parity
    out = fuzz_parity.run(4.0, 20261018, verbose=True, only=["case_blocks_gain"])
    print(out["per_family"], "skipped", out["skipped_geometries"])
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert list(out["per_family"]) == ["case_blocks_gain"] and out["cases"] >= 5 and out["skipped_geometries"] == 0, out


def test_fuzz_slice_resize(gpu):
    """isx_resize and isx_mask_dilate_resize_and's family alone, over its eight shape classes, four types and four placements."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_parity
    out = fuzz_parity.run(4.0, 20261019, verbose=True, only=["case_resize"])
    print(out["per_family"], "skipped", out["skipped_geometries"])
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert list(out["per_family"]) == ["case_resize"] and out["cases"] >= 5 and out["skipped_geometries"] == 0, out


def test_fuzz_slice_graphcut_grad(gpu):
    """GraphCutSeamFinder(COST_COLOR_GRAD)'s family alone, over its seven classes (the structured patterns among them) and four placements:
    masks byte for byte and the 64-bit certificate of the first pair.  Its model is a max-flow on Python ints, about 0.1 s a case."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_parity
    out = fuzz_parity.run(4.0, 20261106, verbose=True, only=["case_graphcut_grad"])
    print(out["per_family"], "skipped", out["skipped_geometries"])
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert list(out["per_family"]) == ["case_graphcut_grad"] and out["cases"] >= 5 and out["skipped_geometries"] == 0, out


def test_fuzz_slice_plan_verify(gpu):
    """The planned warp's ROI verification alone: random cameras of its ten classes with the true plan or one bound of it moved, against the
    three-valued model (0 where it must pass, 1 where it must flag)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_parity
    out = fuzz_parity.run(4.0, 20261107, verbose=True, only=["case_plan_verify"])
    print(out["per_family"], "skipped", out["skipped_geometries"])
    assert out["mismatches"] == 0, out["failing_seeds"]
    assert list(out["per_family"]) == ["case_plan_verify"] and out["cases"] >= 20 and out["skipped_geometries"] * 10 <= out["cases"], out


# seeds the soaks have tripped over, kept as cases of their own (family, seed):
#   case_many_tiles 20260988784363 - round 5: 35 tiles in mode 2, two bands; one column strip of the cycle took k_collapse_gather (16-byte level-1
#   records, produced again on its columns), its neighbour read a shared tile's planar level 1 from feed() behind it
#   case_blocks_gain 20261078783058 - three tiles that all meet: isx_blocks_gain_stats gave the records image pair by image pair, not by (block_i, block_j)
#   case_resize 20261164820493 - a 1 x 72 CV_8UC3 source whose NumPy row stride was 3 (a C-contiguous array keeps any stride on a dimension of
#   length 1): as_mat handed it on as the step and isx_resize refused it ("step 3 smaller than a row"); as_mat now gives one row its bytes
#   case_graphcut_grad 20261166783477 - no soak tripped over it: three tiles in device views, the serpentine against itself flipped, whose first
#   pair (grid 40 x 103) ties - minimal source side 2 166 nodes, maximal 2 563; kept so that a tie under COST_COLOR_GRAD runs with every suite
#   case_plan_verify 20261168960453, 20261169325876 - the south pole inside the image beside its first row and a border that stays on one
#   side of u = 0: the ROI's br.u (tl.u) is the pole's 0, and a planned -1 (1) was compared with the border's own extremum, which it fits
REGRESSIONS = [("case_many_tiles", 20260988784363), ("case_blocks_gain", 20261078783058), ("case_resize", 20261164820493),
               ("case_graphcut_grad", 20261166783477), ("case_plan_verify", 20261168960453), ("case_plan_verify", 20261169325876)]


@pytest.mark.parametrize("family,seed", REGRESSIONS)
def test_fuzz_regression_seed(gpu, family, seed):
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_parity
    fuzz_parity.G.load()
    getattr(fuzz_parity, family)(np.random.default_rng(seed))
