"""The generator of tools/fuzz_polar_warp.py without a GPU: cases are a function of their seed, every class, kind, entry, layout,
interpolation and border mode is drawn, the sizes of the tile_edges class sit on the kernels' tiling constants, the windows stay inside
what an int rectangle and a test's budget allow, and the model evaluates every drawn window (far ones beyond sinf's 2^28 included)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_polar_warp as Z  # noqa: E402
from helpers import polar_np as P  # noqa: E402

FIRST = Z.CLASSES[:5]                       # (the classes of the first sweep keep their seeds)
CASES = [Z.case(7000 + i, FIRST[i % len(FIRST)]) for i in range(400)] + [Z.case(9000 + i, "captured") for i in range(80)]


def test_cases_are_a_function_of_the_seed():
    for c in CASES[:40]:
        d = Z.case(c["seed"], c["cls"])
        assert all(np.array_equal(c[k], d[k]) for k in c)
    assert Z.case(5)["cls"] in Z.CLASSES


def test_every_class_and_switch_is_drawn():
    for key, values in (("cls", Z.CLASSES), ("kind", (P.FISHEYE, P.STEREOGRAPHIC)), ("entry", Z.ENTRIES), ("layout", Z.LAYOUTS), ("interp", Z.INTERPS),
                        ("border", Z.BORDERS), ("rname", tuple(P.ROTATIONS)), ("out16", (False, True)), ("with_mask", (False, True))):
        assert {c[key] for c in CASES} == set(values), key
    assert {(c["cn"], c["dtype"]) for c in CASES} == set(Z.TYPES)
    assert any(c["gain"] != 1.0 for c in CASES if c["cls"] == "fused") and all(c["gain"] == 1.0 for c in CASES if c["with_mask"])


def test_sizes_and_windows():
    edge = [c for c in CASES if c["cls"] == "tile_edges"]
    assert all(min(c["w"] % Z.COL_BLOCK, -c["w"] % Z.COL_BLOCK) <= 1 for c in edge)
    assert all(min(c["h"] % Z.ROW_BLOCK, -c["h"] % Z.ROW_BLOCK) <= 1 for c in edge)
    assert {c["w"] % Z.COL_BLOCK for c in edge} >= {0, 1, Z.COL_BLOCK - 1} and any(c["w"] > Z.SCAN_COLS for c in edge)
    for c in CASES:
        assert c["w"] >= 1 and c["h"] >= 1 and c["scale"] > 0 and np.isfinite(c["K"]).all() and np.isfinite(c["R"]).all()
        assert np.allclose(c["R"].astype(np.float64) @ c["R"].astype(np.float64).T, np.eye(3), atol=1e-5)
        if c["window"] is not None:
            x0, y0, x1, y1 = c["window"]
            assert -2 ** 31 < x0 <= x1 < 2 ** 31 and -2 ** 31 < y0 <= y1 < 2 ** 31 and x1 - x0 < 2 * Z.MAX_WINDOW and y1 - y0 < 2 * Z.MAX_WINDOW
    assert all(c["window"][0] <= 0 <= c["window"][2] and c["window"][1] <= 0 <= c["window"][3] for c in CASES if c["cls"] == "pole_window")
    far = [c for c in CASES if c["cls"] == "far_window"]
    radius = [max(abs(v) for v in c["window"]) / c["scale"] for c in far]
    assert min(radius) < 100 and max(radius) > 2.0 ** 28            # both sides of the range sinf / cosf serve


def test_the_model_evaluates_every_window():
    for c in CASES[:120]:
        if c["window"] is None:
            continue
        m = P.from_rig(c["kind"], c["scale"], c["K"], c["R"])
        xm, ym = m.build_maps(c["window"])
        assert xm.shape == (c["window"][3] - c["window"][1] + 1, c["window"][2] - c["window"][0] + 1) and not np.isnan(xm).any() and not np.isnan(ym).any()
        if max(abs(v) for v in c["window"]) / c["scale"] > 2.0 ** 28 + 200:
            assert ((xm == -1) & (ym == -1)).all()                    # sinf / cosf give NaN out there: z > 0 fails, the sentinel


def test_the_captured_class():
    """device mats, an entry that takes the caller's window (the ROI scan synchronises: never captured), every such entry and both window forms drawn"""
    cap = [c for c in CASES if c["cls"] == "captured"]
    assert len(cap) == 80 and Z.CLASSES[5] == "captured"
    assert all(c["layout"] == "device" and c["entry"] != "roi" for c in cap)
    assert {c["entry"] for c in cap} == {"maps", "warp", "fused"} and {c["window"] is None for c in cap} == {False, True}
    assert {c["kind"] for c in cap} == {P.FISHEYE, P.STEREOGRAPHIC} and {c["with_mask"] for c in cap if c["entry"] == "fused"} == {False, True}
    assert any(c["gain"] != 1.0 for c in cap if c["entry"] == "fused")
