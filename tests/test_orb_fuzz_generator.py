"""The generator of tools/fuzz_orb.py on the CPU: a seed always gives the same case, the classes come in turn, every drawn case is one the
library accepts (its host-side checks run without a GPU) and the model runs on, and the seeds between them reach what the fuzz is for:
every layout, a caller's pattern, several channels and cells, empty results, ties that are truncated."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fuzz_orb as fz  # noqa: E402
from helpers import orb_np as M  # noqa: E402


def test_a_seed_is_a_case():
    a, b = fz.make_case(20261021003), fz.make_case(20261021003)
    assert np.array_equal(a["image"], b["image"]) and a["layout"] == b["layout"] and vars(a["params"]) == vars(b["params"])
    assert (a["pattern"] is None) == (b["pattern"] is None) and (a["pattern"] is None or np.array_equal(a["pattern"], b["pattern"]))
    assert [fz.make_case(s)["cls"] for s in range(10)] == list(fz.CLASSES) * 2
    assert fz.make_case(3, cls="dots")["cls"] == "dots"


def test_the_cases_are_valid_and_reach_the_paths():
    from imagestitch_amd import features
    seen = dict(layouts=set(), channels=set(), patterns=0, cells=set(), empty=0, truncated=0, found=0, levels=set())
    for s in range(60):
        c = fz.make_case(20261021000 + s)
        img, p = c["image"], c["params"]
        assert img.dtype == np.uint8 and 40 <= img.shape[0] <= 330 and 40 <= img.shape[1] <= 330
        assert features.capacity(fz.library_params(p)) == M.capacity(p)              # the library's own parameter checks pass
        assert c["pattern"] is None or M.pattern_ok(c["pattern"])
        r = M.find(img, p, c["pattern"])
        assert r.count <= M.capacity(p) and r.status in (0, M.STATUS_TRUNCATED)
        seen["layouts"].add(c["layout"]); seen["channels"].add(1 if img.ndim == 2 else img.shape[2]); seen["patterns"] += c["pattern"] is not None
        seen["cells"].add(p.grid[0] * p.grid[1]); seen["empty"] += r.count == 0; seen["found"] += r.count > 0; seen["truncated"] += r.status == M.STATUS_TRUNCATED
        seen["levels"] |= set(r.meta[:, 3].astype(int))
    print(seen)
    assert seen["layouts"] == set(fz.LAYOUTS) and seen["channels"] == {1, 3, 4} and seen["patterns"] >= 10 and len(seen["cells"]) >= 4
    assert seen["empty"] >= 5 and seen["found"] >= 15 and seen["truncated"] >= 1 and {0, 1, 2} <= seen["levels"]


def test_a_seed_is_a_case_of_the_limits_family():
    a, b = fz.make_limit_case(20261021003), fz.make_limit_case(20261021003)
    assert np.array_equal(a["image"], b["image"]) and a["layout"] == b["layout"] and vars(a["params"]) == vars(b["params"])
    assert (a["pattern"] is None) == (b["pattern"] is None) and (a["pattern"] is None or np.array_equal(a["pattern"], b["pattern"]))
    assert [fz.make_limit_case(s)["cls"] for s in range(6)] == list(fz.LIMIT_KINDS) * 2
    assert fz.make_limit_case(3, kind="layers")["cls"] == "layers"
    assert fz.FAMILIES["default"] == (fz.make_case, fz.CLASSES) and fz.FAMILIES["limits"] == (fz.make_limit_case, fz.LIMIT_KINDS)


def test_the_limits_family_is_valid_and_reaches_its_paths():
    """over 40 seeds: more than 1024 candidates in a layer (a second pass of k_orb_final_cut), a keypoint in a layer of index >= 256
    (k_orb_describe's second stride), an image under 63 pixels a side; every case is one the library accepts"""
    from imagestitch_amd import features
    seen = dict(layouts=set(), channels=set(), patterns=0, most_candidates=0, last_layer=0, most_layers=0, small=0, empty=0, found=0, truncated=0, one_pixel_cells=0)
    for s in range(40):
        c = fz.make_limit_case(20261021000 + s)
        img, p = c["image"], c["params"]
        h, w = img.shape[:2]
        assert img.dtype == np.uint8 and 1 <= h <= M.MAX_SIDE and 1 <= w <= M.MAX_SIDE and p.grid[0] <= w and p.grid[1] <= h
        assert p.grid[0] * p.grid[1] * p.nlevels <= M.MAX_LAYERS
        assert features.capacity(fz.library_params(p)) == M.capacity(p)              # the library's own parameter checks pass
        if c["cls"] == "passes":
            assert 700 <= p.n_features <= 1920 and p.nlevels in (1, 2)
        elif c["cls"] == "layers":
            assert 64 <= h <= 72 and 64 <= w // p.grid[0] <= 72 and p.grid[1] == 1
        else:
            assert min(h, w) <= 70
        stages = {}
        r = M.find(img, p, c["pattern"], stages=stages)
        assert r.count <= M.capacity(p) and r.status in (0, M.STATUS_TRUNCATED)
        seen["layouts"].add(c["layout"]); seen["channels"].add(1 if img.ndim == 2 else img.shape[2]); seen["patterns"] += c["pattern"] is not None
        seen["most_candidates"] = max([seen["most_candidates"]] + [len(v["candidates"]) for v in stages.values()])
        seen["last_layer"] = max([seen["last_layer"]] + [ci * p.nlevels + l for (ci, l), v in stages.items() if len(v["final"])])
        seen["most_layers"] = max(seen["most_layers"], p.grid[0] * p.grid[1] * p.nlevels)
        seen["small"] += h < 63 or w < 63; seen["empty"] += r.count == 0; seen["found"] += r.count > 0; seen["truncated"] += r.status == M.STATUS_TRUNCATED
        seen["one_pixel_cells"] += w // p.grid[0] == 1 or h // p.grid[1] == 1
    print(seen)
    assert seen["most_candidates"] > 1024 and seen["last_layer"] >= 256 and seen["small"] >= 5
    assert seen["layouts"] == set(fz.LAYOUTS) and seen["channels"] == {1, 3, 4} and seen["patterns"] >= 5
    assert seen["empty"] >= 5 and seen["found"] >= 15 and seen["truncated"] >= 1 and seen["most_layers"] > 512
