"""The limit cases of tests/orb_cases.py on the model alone (no GPU): each reaches the path it is for - more than one pass of
k_orb_final_cut's 1024 candidates, ties decided across the passes, a keypoint in a layer past k_orb_describe's first stride of 256, 1024
layers, the smallest sides and ISX_ORB_MAX_SIDE - so that a case cannot drift into testing nothing.  The conditions are asserted, the
model's own figures and seconds are printed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_cases as cases  # noqa: E402
from helpers import orb_np as M  # noqa: E402

ERR_UNSUPPORTED = 6
PASS = 1024                                                 # OB_CUT_NT: the candidates a pass of k_orb_final_cut takes


def model(name):
    img, p, want, stages, seconds = cases.limit_want(name)
    print("%s: %d x %d, count %d, status %d, the model took %.2f s" % (name, img.shape[0], img.shape[1], want.count, want.status, seconds))
    assert seconds < 5.0, (name, seconds)
    assert want.count <= M.capacity(p)
    return img, p, want, stages


def layers_with_keypoints(p, stages):
    """layer index = cell * nlevels + level of every layer whose final set is not empty"""
    return sorted(ci * p.nlevels + l for (ci, l), s in stages.items() if len(s["final"]))


@pytest.mark.parametrize("name,passes,count", [("passes-2", 2, 1500), ("passes-4", 4, 1920)])
def test_noise_fills_more_than_one_pass(name, passes, count):
    _, p, want, stages = model(name)
    m = len(stages[(0, 0)]["candidates"])
    print(name, "candidates", m)
    assert list(stages) == [(0, 0)] and (passes - 1) * PASS < m <= passes * PASS
    assert m <= 2 * p.n_features + M.CAND_TIE_ROOM <= M.MAX_CANDIDATES
    assert want.count == count and want.status == 0
    resp = stages[(0, 0)]["responses"]
    assert len(np.unique(resp)) > m // 2                    # the responses decide, not the ties
    # the kept rows come from every pass, and rows of a later pass are kept while rows of the first are dropped
    final = stages[(0, 0)]["final"]
    assert set(final // PASS) == set(range(passes)) and len(final) < m


def test_1921_features_on_a_level_are_unsupported():
    from imagestitch_amd import _lib, features
    q = features.default_params()
    q.grid_width = q.grid_height = q.nlevels = 1
    q.n_features = 1920
    assert features.capacity(q) == 1920 + M.KEEP_TIE_ROOM
    q.n_features = 1921
    with pytest.raises(_lib.IsxError) as e:
        features.capacity(q)
    assert e.value.code == ERR_UNSUPPORTED, e.value


@pytest.mark.parametrize("name,candidates,kept,status", [("passes-ties-fit", 1100, 1100, 0), ("passes-ties-cut", 1300, 1232, M.STATUS_TRUNCATED),
                                                         ("passes-ties-full", 3025, 1932, M.STATUS_TRUNCATED)])
def test_equal_responses_are_cut_across_the_passes(name, candidates, kept, status):
    _, p, want, stages = model(name)
    s = stages[(0, 0)]
    assert len(s["candidates"]) == candidates > PASS and want.count == kept and want.status == status
    assert kept == min(candidates, p.n_features + M.KEEP_TIE_ROOM) > PASS
    assert len(np.unique(s["responses"].view(np.uint32))) == 1                      # one response: equal_before alone decides a row
    assert np.array_equal(s["final"], np.arange(kept))                              # the first `kept` in canonical order, past row 1024
    assert s["truncated"] == (False, status != 0)


@pytest.mark.parametrize("name,layers,beyond,non_empty", [("layers-264", 264, 256, 50), ("layers-1024", 1024, 1000, 200)])
def test_strips_hold_keypoints_in_layers_past_256(name, layers, beyond, non_empty):
    _, p, want, stages = model(name)
    assert p.grid[0] * p.grid[1] * p.nlevels == layers and len(stages) == layers
    full = layers_with_keypoints(p, stages)
    print(name, "layers with keypoints", len(full), "the last", full[-1], "count", want.count)
    assert full[-1] >= beyond and len(full) > non_empty
    assert sum(i >= 256 for i in full) >= 1 and sum(i < 256 for i in full) > 50     # rows on both sides of the first stride
    assert want.count == sum(len(s["final"]) for s in stages.values()) > 0
    if layers == 1024:
        assert all(sum(1 for i in full if 256 * k <= i < 256 * (k + 1)) > 10 for k in range(4))       # every stride of 256 has its own


@pytest.mark.parametrize("name,count", [("side-1x1", 0), ("side-1x200", 0), ("side-200x1", 0), ("side-62x62", 0), ("side-62x62-dot", 0), ("side-63x63", 1),
                                        ("side-63x200", 18), ("side-3x5-cells-of-1", 0)])
def test_the_smallest_sides(name, count):
    img, p, want, stages = model(name)
    assert want.count == count and want.status == 0
    if name == "side-63x63":
        assert np.array_equal(want.keypoints, [[31, 31]]) and want.meta[0, 3] == 0
    if name == "side-63x200":
        assert (want.keypoints[:, 1] == 31).all() and want.keypoints[0, 0] == 31 and want.keypoints[-1, 0] == 200 - 33
    if name == "side-62x62-dot":
        assert img[30, 30] != img[0, 0]
    if name == "side-3x5-cells-of-1":
        assert img.shape == (3, 5) and p.grid == (5, 3) and M.capacity(p) == 1920
        scales = M.level_scales(p.scale_factor, p.nlevels)
        assert [M.layer_size(1, 1, s) for s in scales] == [(1, 1), (1, 1), (1, 1), (0, 0)]      # the top level rounds to nothing
    assert set(cases.SIDE_CASES) == {n for n in cases.LIMIT_CASES if n.startswith("side-")} and name in cases.SIDE_CASES


@pytest.mark.parametrize("name,axis", [("max-side-x", 0), ("max-side-y", 1)])
def test_the_largest_side(name, axis):
    img, p, want, stages = model(name)
    assert max(img.shape) == 16384 and min(img.shape) == 64 and img.shape[1 - axis] == 16384
    print(name, "count", want.count, "least coordinate", want.keypoints[:, axis].min())
    assert want.count > 0 and want.status == 0 and want.keypoints[:, axis].min() > 16000
    assert want.keypoints[:, axis].max() == 16384 - 32                                           # the last pixel inside the border
    assert (want.meta[:, 3] == 0).all() and stages[(0, 1)]["candidates"].shape[0] == 0           # level 1 is 49 pixels high: nothing


def test_every_limit_case_is_asserted_here():
    named = set()
    for f in (test_noise_fills_more_than_one_pass, test_equal_responses_are_cut_across_the_passes, test_strips_hold_keypoints_in_layers_past_256,
              test_the_smallest_sides, test_the_largest_side):
        for mark in f.pytestmark:
            named |= {args[0] for args in mark.args[1]}
    assert named == set(cases.LIMIT_CASES), named ^ set(cases.LIMIT_CASES)
