"""tools/fuzz_surf.py's generator without a GPU: a seed gives one case, every class sits on the constant it is named after, and the model
answers every class within the time a 5-second slice leaves it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_surf as F  # noqa: E402
from helpers import surf_np as M  # noqa: E402

SEED = 20261201


def test_a_seed_is_a_case():
    for n in range(10):
        s, cls = F.scheduled(SEED, n)
        a, b = F.case(s, cls), F.case(s, cls)
        assert a["cls"] == cls == F.CLASSES[n % len(F.CLASSES)] and np.array_equal(a["image"], b["image"]) and a["params"] == b["params"]
        assert a["layout_seed"] == b["layout_seed"] and a["image"].dtype == np.uint8 and max(a["image"].shape[:2]) <= F.MAX_SIDE
    assert not np.array_equal(F.case(1, "cap")["image"], F.case(2, "cap")["image"])


def test_layer_edges_sit_on_the_filter_sizes():
    seen = set()
    for s in range(60):
        c = F.case(s, "layer_edges")
        all_sizes = F.layer_sizes(c["params"]["num_octaves"], c["params"]["num_layers"])
        d = min(abs(c["side"] - v) for v in all_sizes)
        assert d <= 1 and c["side"] in c["image"].shape[:2]
        seen.add(c["side"] - min(all_sizes, key=lambda v: abs(c["side"] - v)))
    assert seen == {-1, 0, 1}
    assert F.layer_sizes(3, 4) == sorted({(9 + 6 * l) << o for o in range(3) for l in range(6)})


def test_border_class_has_windows_that_leave_the_image():
    left = 0
    for s in range(6):
        c = F.case(s, "border")
        h, w = c["image"].shape
        assert all(min(y, x, h - 1 - y, w - 1 - x) <= 14 for y, x in c["centres"])
        r = M.find(c["image"], M.Params(**c["params"]))
        for (x, y), size in zip(r["keypoints"], r["meta"][:, 0]):
            half = int(21 * M.scale_of(size)) * 0.5 * np.sqrt(2.0)
            left += int(min(x, y, w - 1 - x, h - 1 - y) < half)
    assert left >= 6, left


def test_scales_class_spans_the_layers():
    lo, hi = [], []
    for s in range(4):
        c = F.case(s, "scales")
        assert min(c["image"].shape) >= c["top"] + 4
        r = M.find(c["image"], M.Params(**c["params"]))
        assert r["count"] >= 2
        lo.append(r["meta"][:, 0].min()); hi.append(r["meta"][:, 0].max() / c["top"])
    print(lo, hi)
    assert min(lo) <= 12 and max(hi) >= 0.6            # sizes near 9 (15 - 6 at the least) and near the largest layer


def test_cap_rules_and_the_slice_budget():
    rules = {F.case(s, "cap")["cap_rule"] for s in range(40)}
    assert rules == {"one", "count-1", "count", "count+1"}
    assert [F.cap_of(r, 7) for r in ("room", "one", "count-1", "count", "count+1")] == [10, 1, 6, 7, 8] and F.cap_of("count-1", 0) == 1
    c = F.case(5, "cap")
    c["cap_rule"] = "count-1"
    cap, want = F.expected(c)
    assert want["count"] == cap and want["status"] == M.STATUS_TRUNCATED and want["descriptors"].shape == (cap, 64)
    # one case of every class: generator and model together stay well inside a 5-second slice
    t0 = time.time()
    for n in range(len(F.CLASSES)):
        F.expected(F.case(*F.scheduled(SEED, n)))
    spent = time.time() - t0
    print("one round of the classes: %.2f s" % spent)
    assert spent < 4.0
    channels = {1 if F.case(s, "params")["image"].ndim == 2 else F.case(s, "params")["image"].shape[2] for s in range(30)}
    assert channels == {1, 3, 4}
