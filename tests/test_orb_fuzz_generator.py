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
