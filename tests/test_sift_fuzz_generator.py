"""tools/fuzz_sift.py's generator without a GPU: a seed gives one case, every class sits on the constant it is named after, and the model
answers every class within the time a 5-second slice leaves it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_sift as F  # noqa: E402
from helpers import sift_np as M  # noqa: E402

SEED = 20261221


def test_a_seed_is_a_case():
    for n in range(10):
        s, cls = F.scheduled(SEED, n)
        a, b = F.case(s, cls), F.case(s, cls)
        assert a["cls"] == cls == F.CLASSES[n % len(F.CLASSES)] and np.array_equal(a["image"], b["image"]) and a["params"] == b["params"]
        assert a["layout_seed"] == b["layout_seed"] and a["image"].dtype == np.uint8 and max(a["image"].shape[:2]) <= F.MAX_SIDE
    assert not np.array_equal(F.case(1, "cap")["image"], F.case(2, "cap")["image"])


def test_tiles_sit_on_the_blur_tile():
    seen = set()
    for s in range(60):
        c = F.case(s, "tiles")
        d = min(abs(c["side"] - v) for v in F.TILE_SIDES)
        assert d <= 1 and c["side"] in c["image"].shape[:2]
        seen.add(c["side"] - min(F.TILE_SIDES, key=lambda v: abs(c["side"] - v)))
    assert seen == {-1, 0, 1} and all((2 * v) % 64 == 0 for v in F.TILE_SIDES)


def test_octave_sides_are_where_the_plan_changes():
    """at every listed side the integer octave rule steps, or the octaves that are built differ from those one pixel below"""
    for side in F.OCTAVE_SIDES:
        steps = M.octave_count(2 * side) != M.octave_count(2 * side - 2)
        assert steps or len(M.octave_sizes(side, 200)) != len(M.octave_sizes(side - 1, 200)), side
    assert [s for s in F.OCTAVE_SIDES if M.octave_count(2 * s) != M.octave_count(2 * s - 2)] == [3, 6, 12, 23, 46, 91]
    assert [s for s in F.OCTAVE_SIDES if len(M.octave_sizes(s, 200)) != len(M.octave_sizes(s - 1, 200))] == [6, 11, 22, 44, 88]
    seen = set()
    for s in range(80):
        c = F.case(s, "octaves")
        assert c["side"] in c["image"].shape[:2]
        seen.add(c["side"])
    assert len(seen) >= 12 and {3, 6, 11}.issubset(seen | {v + 1 for v in seen} | {v - 1 for v in seen})


def test_border_class_reaches_the_first_and_last_searched_rows():
    edge = 0
    for s in range(6):
        c = F.case(s, "border")
        h, w = c["image"].shape
        assert all(min(y, x, h - 1 - y, w - 1 - x) <= 4.25 for y, x in c["centres"])
        t = {}
        M.find(c["image"], M.Params(**c["params"]), None, t)
        cand = t["candidates"]
        for o, r, col in zip(cand["octave"], cand["r"], cand["c"]):
            rows, cols = t["octaves"][int(o)]
            edge += int(min(r, col, rows - 1 - r, cols - 1 - col) <= M.BORDER + 1)
    assert edge >= 6, edge


def test_cap_rules_and_the_slice_budget():
    rules = {F.case(s, "cap")["cap_rule"] for s in range(60)}
    assert rules == {"one", "count-1", "count", "count+1", "nf-1", "nf+1"}
    assert [F.cap_of(r, 7) for r in ("room", "one", "count-1", "count", "count+1", "nf-1")] == [10, 1, 6, 7, 8, 10] and F.cap_of("count-1", 0) == 1
    c = F.case(5, "cap")
    c["cap_rule"] = "count-1"
    cap, nf, want = F.expected(c)
    assert want["count"] == cap and nf == 0 and want["status"] == M.STATUS_TRUNCATED and want["descriptors"].shape == (cap, 128)
    c["cap_rule"] = "nf-1"
    cap, nf, want = F.expected(c)
    assert want["count"] == nf == cap - 4 and want["status"] == 0
    # one case of every class: generator and model together stay well inside a 5-second slice
    t0 = time.time()
    for n in range(len(F.CLASSES)):
        F.expected(F.case(*F.scheduled(SEED, n)))
    spent = time.time() - t0
    print("one round of the classes: %.2f s" % spent)
    assert spent < 4.0
    channels = {1 if F.case(s, "params")["image"].ndim == 2 else F.case(s, "params")["image"].shape[2] for s in range(30)}
    assert channels == {1, 3, 4}
