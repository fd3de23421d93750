"""Structured inputs for GraphCutSeamFinder (both cost types): two tiles of constant, ramp, step, checkerboard and serpentine images, on
which minimum cuts tie and the capacities sit at the ends of their range - what the random layout() tiles of the graph-cut suites never
give.  NumPy only.  tests/test_graphcut_structured_model.py proves on the models what each case is (tie or unique, range of weights) and
keeps the recorded answers; tests/test_gpu_graphcut_structured.py runs them on the GPU; the patterns themselves are tools/graphcut_patterns.py, from which
tools/fuzz_parity.py draws as well.

    structured_pair(name, size) -> (imgs, corners, masks)       name in PATTERNS (either size) or MASK_VARIANTS ("small" only)
    terminal_pair(name)         -> (imgs, corners, masks)       name in TERMINALS: graphs without a source or a sink terminal
    small_case(name)            -> (imgs, corners, masks)       name in SMALL_CASES: every small case by one name, the strips included
Images are uint8 (callers convert to float32); masks are 255 unless the case says otherwise."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from graphcut_patterns import PATTERNS, pattern_images, serpentine  # noqa: E402,F401  (shared with tools/fuzz_parity.py)

# tile (rows, cols), the two corners (x, y), the padded grid (rows, cols) = (overlap + 2 * 10)
SIZES = {"small": ((40, 70), ((0, 0), (30, 3)), (57, 60)),
         "wide": ((60, 260), ((0, 0), (40, 3)), (77, 240))}       # 5 x 4 of the 64 x 16 BFS tiles

MASK_VARIANTS = ("holes", "odd_bytes")                            # both on VARIANT_PATTERN
VARIANT_PATTERN = "ramp_rev"
TERMINALS = ("full_empty", "empty_full", "full_full", "empty_empty")
STRIPS = ("strip_0", "strip_30")
SMALL_CASES = PATTERNS + MASK_VARIANTS + TERMINALS + STRIPS

# Measured by tests/test_graphcut_structured_model.py, which asserts all of it: in a tie the minimal and the maximal source side of the
# maximum flow differ (and cost the same); in a unique case they are one set.  TIE_CASES tie under both cost types, UNIQUE_CASES under
# neither, and TIE_UNDER_ONE names the one cost type (0 = COST_COLOR, 1 = COST_COLOR_GRAD) under which a case ties: the gradients of a
# ramp break COST_COLOR's ties, and those of a step make some.
TIE_CASES = ("identical", "const_10_13", "xramp_yramp", "checker_inv", "serp_0", "serp_serp", "channels", "full_full", "empty_empty", "strip_0")
UNIQUE_CASES = ("const_0_255", "full_empty", "empty_full", "strip_30")
TIE_UNDER_ONE = {"ramp_rev": 0, "holes": 0, "odd_bytes": 0, "step_inv": 1}


def is_tie(name, cost_type):
    return name in TIE_CASES or TIE_UNDER_ONE.get(name) == cost_type


def structured_pair(name, size="small"):
    (h, w), corners, grid = SIZES[size]
    masks = [np.full((h, w), 255, np.uint8) for _ in range(2)]
    if name in MASK_VARIANTS:
        assert size == "small", "the mask variants exist at the small size only"
        imgs = pattern_images(VARIANT_PATTERN, h, w)
        if name == "holes":
            # (tile, y, x, rows, cols); the overlap is x 30..70, y 3..40 of tile 0 and x 0..40, y 0..37 of tile 1
            holes = ((0, 10, 40, 6, 9), (0, 0, 5, 4, 7), (0, 33, 60, 7, 10), (1, 20, 12, 5, 11), (1, 30, 50, 6, 8), (1, 2, 33, 9, 4))
            (x0, y0), (x1, y1) = corners
            ox, oy = max(x0, x1), max(y0, y1)
            ow, oh = min(x0, x1) + w - ox, min(y0, y1) + h - oy
            inside = 0
            for t, y, x, r, c in holes:
                masks[t][y:y + r, x:x + c] = 0
                gx, gy = x + corners[t][0], y + corners[t][1]
                inside += ox <= gx and gx + c <= ox + ow and oy <= gy and gy + r <= oy + oh
            assert inside >= 1 and all((m == 0).any() for m in masks)
        else:                                                     # set bytes 1, 128 and 254 in stripes of columns
            for m in masks:
                m[:, :] = np.array([1, 128, 254], np.uint8)[(np.arange(w) // 5) % 3][None, :]
    else:
        imgs = pattern_images(name, h, w)
    return imgs, list(corners), masks


def terminal_pair(name):
    """Two identical 12 x 14 tiles at the same corner with (mask 1, mask 2) full or empty: no source terminal, no sink terminal, or neither
    (tests/test_graphcut_model.py test_a_graph_without_source_or_sink_terminals)."""
    a, b = name.split("_")
    img = np.full((12, 14, 3), 50, np.uint8)
    mk = {"full": np.full((12, 14), 255, np.uint8), "empty": np.zeros((12, 14), np.uint8)}
    return [img, img.copy()], [(0, 0), (0, 0)], [mk[a].copy(), mk[b].copy()]


def small_case(name):
    if name in STRIPS:
        from test_graphcut_model import strip
        return strip(int(name.split("_")[1]))
    if name in TERMINALS:
        return terminal_pair(name)
    return structured_pair(name, "small")
