"""The structured cases of tests/graphcut_cases.py on the two NumPy models alone (graphcut_np: COST_COLOR, graphcut_grad_np: COST_COLOR_GRAD):
what tests/test_gpu_graphcut_structured.py relies on is proved here without a GPU.  Every small case is solved by the model's own max_flow
under both cost types: the certificate holds, the case ties (minimal source side != maximal, same capacity) or is unique as
graphcut_cases records it, the capacities reach the ends of their range (390 151 on constant 0 against 255, all-1 on identical tiles,
rounded quotients on the ramps), mask bytes 1, 128 and 254 count as set, and flow, label count and mask bytes are the recorded KNOWN.  The
wide cases only build their graph."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphcut_cases as GC  # noqa: E402
from helpers import graphcut_grad_np as GG  # noqa: E402
from helpers import graphcut_np as G  # noqa: E402

COLOR, GRAD = GG.COST_COLOR, GG.COST_COLOR_GRAD
COSTS = [COLOR, GRAD]
UNIT = {COLOR: 1, GRAD: GG.SCALE}


def roi_of(imgs, corners):
    return G.overlap_roi(corners[0], corners[1], *[(a.shape[1], a.shape[0]) for a in imgs])


@functools.lru_cache(maxsize=None)
def solved(name, cost_type):
    """(graph, flow, certificate, masks after the write-back) of a small case: solved once, shared, read-only."""
    if cost_type == COLOR:
        pytest.importorskip("scipy")
    imgs, corners, masks = GC.small_case(name)
    roi = roi_of(imgs, corners)
    g = GG.pair_graph(imgs[0], imgs[1], masks[0], masks[1], corners[0], corners[1], roi, cost_type)
    flow, cert = (GG.max_flow if cost_type == GRAD else G.max_flow)(g)
    out = [m.copy() for m in masks]
    G.write_back(cert["labels"], out[0], out[1], corners[0], corners[1], roi)
    for a in list(g.values()) + list(cert.values()) + out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return g, flow, cert, tuple(out)


def unpenalised(g, imgs, corners, masks):
    """The right and down capacities of the edges whose four mask bytes are set."""
    roi = roi_of(imgs, corners)
    ok = (G._cut(masks[0], corners[0], roi, ()) != 0) & (G._cut(masks[1], corners[1], roi, ()) != 0)
    return np.concatenate([g["right"][:, :-1][ok[:, :-1] & ok[:, 1:]], g["down"][:-1][ok[:-1] & ok[1:]]])


# (case, cost type): (flow, nodes on the maximal source side, bytes left in the two masks)
KNOWN = {
    ('identical', 0): (54099, 2458, [2726, 1394]),
    ('const_10_13', 0): (29002, 2364, [2724, 1396]),
    ('const_0_255', 0): (867097, 793, [1320, 2800]),
    ('ramp_rev', 0): (2039391, 1791, [2060, 2060]),
    ('xramp_yramp', 0): (2366241, 2206, [2448, 1672]),
    ('step_inv', 0): (1342072, 568, [1320, 2800]),
    ('checker_inv', 0): (414249, 2459, [2726, 1394]),
    ('serp_0', 0): (291113, 2530, [2757, 1363]),
    ('serp_serp', 0): (350112, 2381, [2700, 1420]),
    ('channels', 0): (857202, 933, [1344, 2776]),
    ('holes', 0): (2797373, 1766, [2025, 2019]),
    ('odd_bytes', 0): (2039391, 1791, [2060, 2060]),
    ('full_empty', 0): (0, 1088, [168, 0]),
    ('empty_full', 0): (0, 0, [0, 168]),
    ('full_full', 0): (0, 1088, [168, 0]),
    ('empty_empty', 0): (0, 1088, [0, 0]),
    ('strip_0', 0): (8008, 480, [6, 3]),
    ('strip_30', 0): (8008, 3, [3, 6]),
    ('identical', 1): (453815304192, 2458, [2726, 1394]),
    ('const_10_13', 1): (243286409216, 2364, [2724, 1396]),
    ('const_0_255', 1): (7273736830976, 793, [1320, 2800]),
    ('ramp_rev', 1): (7034668353388, 1710, [2060, 2060]),
    ('xramp_yramp', 1): (571923294942, 1309, [1568, 2552]),
    ('step_inv', 1): (8365556629504, 932, [1344, 2776]),
    ('checker_inv', 1): (3474972475392, 2459, [2726, 1394]),
    ('serp_0', 1): (185518783738, 2440, [2690, 1430]),
    ('serp_serp', 1): (185367789568, 2340, [2690, 1430]),
    ('channels', 1): (6183679688704, 932, [1344, 2776]),
    ('holes', 1): (9783264436789, 1631, [1905, 2139]),
    ('odd_bytes', 1): (7034668353388, 1710, [2060, 2060]),
    ('full_empty', 1): (0, 1088, [168, 0]),
    ('empty_full', 1): (0, 0, [0, 168]),
    ('full_full', 1): (0, 1088, [168, 0]),
    ('empty_empty', 1): (0, 1088, [0, 0]),
    ('strip_0', 1): (67175972864, 480, [6, 3]),
    ('strip_30', 1): (67175972864, 3, [3, 6]),
}


def test_the_lists_cover_every_small_case_once():
    names = list(GC.TIE_CASES) + list(GC.UNIQUE_CASES) + list(GC.TIE_UNDER_ONE)
    assert sorted(names) == sorted(GC.SMALL_CASES) and len(set(names)) == len(names)
    assert sorted(KNOWN) == sorted((n, c) for n in GC.SMALL_CASES for c in COSTS)
    for cost in COSTS:
        assert sum(GC.is_tie(n, cost) for n in GC.SMALL_CASES) >= 5


@pytest.mark.parametrize("size", sorted(GC.SIZES))
def test_geometry(size):
    (h, w), corners, grid = GC.SIZES[size]
    for name in GC.PATTERNS + (GC.MASK_VARIANTS if size == "small" else ()):
        imgs, cs, masks = GC.structured_pair(name, size)
        assert all(a.shape == (h, w, 3) and a.dtype == np.uint8 for a in imgs) and all(m.shape == (h, w) and m.dtype == np.uint8 for m in masks)
        assert (np.array_equal(imgs[0][..., 0], imgs[0][..., 1]) and np.array_equal(imgs[1][..., 1], imgs[1][..., 2])) == (name != "channels")
        roi = roi_of(imgs, cs)
        assert (roi[3] + 2 * G.GAP, roi[2] + 2 * G.GAP) == grid
    s = GC.serpentine(12, 9)
    assert s[1].all() and s[5].all() and s[9].all() and not s[0].any()
    assert s[2:5, 8].all() and not s[2:5, :8].any() and s[6:9, 0].all() and not s[6:9, 1:].any()


@pytest.mark.parametrize("cost_type", COSTS)
@pytest.mark.parametrize("name", GC.SMALL_CASES)
def test_small_case(name, cost_type):
    g, flow, cert, out = solved(name, cost_type)
    G.check_certificate(g, flow, cert["residuals"], cert["labels"])
    low = G.minimal_source_side(g, cert["residuals"])
    assert G.cut_capacity(g, low) == G.cut_capacity(g, cert["labels"]) == flow
    assert (not np.array_equal(low, cert["labels"])) == GC.is_tie(name, cost_type)
    if GC.is_tie(name, cost_type):
        assert (low <= cert["labels"]).all() and low.sum() < cert["labels"].sum()       # the minimal side lies inside the maximal one
    assert (flow, int(cert["labels"].sum()), [int(np.count_nonzero(m)) for m in out]) == KNOWN[(name, cost_type)]
    # find() is the pair's write-back
    imgs, corners, masks = GC.small_case(name)
    got = GG.find([a.astype(np.float32) for a in imgs], corners, [m.copy() for m in masks], cost_type)
    assert np.array_equal(got[0], out[0]) and np.array_equal(got[1], out[1])


@pytest.mark.parametrize("cost_type", COSTS)
def test_range_of_the_capacities(cost_type):
    unit = UNIT[cost_type]
    g = solved("const_0_255", cost_type)[0]
    w = unpenalised(g, *GC.small_case("const_0_255"))
    assert w.size and (w == 390151 * unit).all()                                 # 2 * 3 * 255^2 + 1: 39 times a terminal link
    assert 390151 << 23 > 1 << 41 and max(g["src"].max(), g["snk"].max()) == 10000 * unit
    g = solved("identical", cost_type)[0]
    w = unpenalised(g, *GC.small_case("identical"))
    assert w.size and (w == unit).all()
    for name in ("ramp_rev", "xramp_yramp"):
        g = solved(name, GRAD)[0]
        w = unpenalised(g, *GC.small_case(name))
        assert (w & ((1 << 10) - 1) != 0).any(), name                            # a rounded quotient: low bits of the Q23 word are set
        assert (w >= 1 << 23).all()
    g, flow, cert, out = solved("odd_bytes", cost_type)
    imgs, corners, masks = GC.small_case("odd_bytes")
    assert sorted(np.unique(np.concatenate(masks)).tolist()) == [1, 128, 254]
    roi = roi_of(imgs, corners)
    full = [np.full_like(m, 255) for m in masks]
    want = GG.pair_graph(imgs[0], imgs[1], full[0], full[1], corners[0], corners[1], roi, cost_type)
    assert all(np.array_equal(g[k], want[k]) for k in ("src", "snk", "right", "down"))
    assert np.array_equal(cert["labels"], solved(GC.VARIANT_PATTERN, cost_type)[2]["labels"])


@pytest.mark.parametrize("cost_type", COSTS)
def test_wide_graphs_build(cost_type):
    for name in GC.PATTERNS:
        imgs, corners, masks = GC.structured_pair(name, "wide")
        g = GG.pair_graph(imgs[0], imgs[1], masks[0], masks[1], corners[0], corners[1], roi_of(imgs, corners), cost_type)
        assert g["src"].shape == (77, 240) and g["src"].any() and g["snk"].any()
        assert min(g["right"][:, :-1].min(), g["down"][:-1].min()) >= UNIT[cost_type]


def test_terminal_free_graphs_and_strips_are_the_model_suites():
    """The four terminal cases are those of test_a_graph_without_source_or_sink_terminals, the strips those of test_graphcut_model."""
    for name, src_side in (("full_empty", True), ("empty_full", False), ("full_full", True), ("empty_empty", True)):
        for cost in COSTS:
            g, flow, cert, out = solved(name, cost)
            _, _, masks = GC.small_case(name)
            assert flow == 0 and (cert["labels"] == (1 if src_side else 0)).all() and g["src"].shape == (32, 34)
            assert np.array_equal(out[0], masks[0]) and np.array_equal(out[1], np.zeros_like(masks[1]) if (src_side and masks[0].any()) else masks[1])
    for cost in COSTS:
        assert solved("strip_0", cost)[1] == solved("strip_30", cost)[1] == 8008 * UNIT[cost]
        assert [m.tolist() for m in solved("strip_0", cost)[3]] == [[[255] * 6], [[0, 0, 0, 255, 255, 255]]]
        assert [m.tolist() for m in solved("strip_30", cost)[3]] == [[[255, 255, 255, 0, 0, 0]], [[255] * 6]]


def test_the_models_refuse_what_the_value_check_refuses():
    """Every value tests/test_gpu_graphcut_structured.py expects the GPU to refuse, the denormal and the float just above 255 included; -0.0
    is accepted and reads as 0."""
    for v in BAD_VALUES:
        bad = np.zeros((4, 4, 3), np.float32)
        bad[1, 2, 0] = v
        with pytest.raises(G.Unsupported):
            G.as_int_image(bad)
        for cost in COSTS:
            with pytest.raises(G.Unsupported):
                GG.find([np.zeros((4, 4, 3), np.float32), bad], [(0, 0), (2, 2)], [np.full((4, 4), 255, np.uint8) for _ in range(2)], cost)
    assert not G.as_int_image(np.full((2, 2, 3), -0.0, np.float32)).any()


BAD_VALUES = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-1), np.float32(256), np.float32(0.5), np.float32(254.5),
              np.nextafter(np.float32(255), np.float32(np.inf)), np.float32(1e-40)]
