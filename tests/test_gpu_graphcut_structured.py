"""GraphCutSeamFinder on the GPU where its suites never went: the structured cases of tests/graphcut_cases.py, whose minimum cuts tie and
whose capacities sit at the ends of the int32 / int64 Q23 range (tests/test_graphcut_structured_model.py proves that on the models), graphs
without a source or a sink terminal (the first global relabel finds nothing active and no round runs), the hand-worked strips, the
CV_32FC3 value check at every kind of bad value, place, tile and entry, and the 2^26-node refusal of COST_COLOR_GRAD.

Every structured case goes through the 64-bit certificate (check_pair of tests/test_gpu_graphcut_grad.py): the residuals prove a maximum
flow of the model's graph, every capacity bit for bit, and the labels its MAXIMAL source side; on a tie the labels are also asserted to
differ from the minimal source side, which a kernel returning another minimum cut would give.

test_value_check runs the full cross product (9 values x 2 places x 4 tiles x find / pair entry x host / device mats) under both cost
types.  test_grid_limit_refusal runs the refused side of the 2^26-node limit only: the accepted side is a 3.2 GB graph and minutes of
run time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphcut_cases as GC  # noqa: E402
from helpers import graphcut_grad_np as GG  # noqa: E402
from helpers import graphcut_np as G  # noqa: E402
from helpers import guarded  # noqa: E402
from test_gpu_graphcut_grad import _dev, _f32, _np, check_pair  # noqa: E402
from test_graphcut_structured_model import BAD_VALUES, KNOWN, solved  # noqa: E402

pytestmark = pytest.mark.gpu
COLOR, GRAD = GG.COST_COLOR, GG.COST_COLOR_GRAD
MODES = {"color_u8": (COLOR, False), "color_f32": (COLOR, True), "grad": (GRAD, True)}


def _src(imgs, f32):
    return _f32(imgs) if f32 else [a.copy() for a in imgs]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", GC.SMALL_CASES)
def test_structured_small(gpu, name, mode):
    cost, f32 = MODES[mode]
    imgs, corners, masks = GC.small_case(name)
    g, flow, cert, want = solved(name, cost)
    src = _src(imgs, f32)
    m = [x.copy() for x in masks]
    r = check_pair(gpu, src[0], src[1], corners[0], corners[1], m[0], m[1], cost_type=cost)
    print(name, mode, "rounds", r["rounds"], "launches", r["launches"])
    assert (r["rows"], r["cols"]) == g["src"].shape
    assert (r["flow"], int(r["labels"].sum()), [int(np.count_nonzero(x)) for x in m]) == KNOWN[(name, cost)] and r["flow"] == flow
    assert np.array_equal(r["labels"], cert["labels"])
    assert np.array_equal(m[0], want[0]) and np.array_equal(m[1], want[1])
    dm = [_dev(x) for x in masks]
    gpu.GraphCutSeamFinder(cost_type=cost).find([_dev(a) for a in src], corners, dm)
    assert np.array_equal(_np(dm[0]), want[0]) and np.array_equal(_np(dm[1]), want[1])
    if GC.is_tie(name, cost):
        low = G.minimal_source_side(g, cert["residuals"])
        assert not np.array_equal(r["labels"], low) and G.cut_capacity(g, low) == r["flow"]     # another minimum cut, not the one returned


@pytest.mark.parametrize("cost", [COLOR, GRAD])
@pytest.mark.parametrize("name", GC.PATTERNS)
def test_structured_wide(gpu, name, cost):
    """77 x 240: 5 x 4 BFS tiles, so a global relabel crosses tiles and needs more than one batch of launches.  The certificate alone
    proves the flow and the maximal cut: no CPU solve."""
    imgs, corners, masks = GC.structured_pair(name, "wide")
    src = _f32(imgs)
    r = check_pair(gpu, src[0], src[1], corners[0], corners[1], masks[0], masks[1], cost_type=cost)
    print(name, cost, "rounds", r["rounds"], "launches", r["launches"])
    assert (r["rows"], r["cols"]) == (77, 240)
    assert r["flow"] > 0 and 0 < int(r["labels"].sum()) < 77 * 240


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name,src_side", [("full_empty", True), ("empty_full", False), ("full_full", True), ("empty_empty", True)])
def test_terminal_free_graphs(gpu, name, src_side, mode):
    """No sink link (or no terminal at all): flow 0, every node on the source side, and the round loop never runs; no source link: flow
    0, every node reaches the sink.  Masks as tests/test_graphcut_model.py test_a_graph_without_source_or_sink_terminals states them."""
    cost, f32 = MODES[mode]
    imgs, corners, masks = GC.terminal_pair(name)
    src = _src(imgs, f32)
    m = [x.copy() for x in masks]
    r = check_pair(gpu, src[0], src[1], corners[0], corners[1], m[0], m[1], cost_type=cost)
    assert r["flow"] == 0 and r["rounds"] == 0 and (r["rows"], r["cols"]) == (32, 34)
    assert (r["labels"] == (1 if src_side else 0)).all()
    assert np.array_equal(m[0], masks[0])
    assert np.array_equal(m[1], np.zeros_like(masks[1]) if (src_side and masks[0].any()) else masks[1])
    dm = [_dev(x) for x in masks]
    gpu.GraphCutSeamFinder(cost_type=cost).find([_dev(a) for a in src], corners, dm)
    assert np.array_equal(_np(dm[0]), m[0]) and np.array_equal(_np(dm[1]), m[1])


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("d2,mask1,mask2,labels", [(0, [255] * 6, [0, 0, 0, 255, 255, 255], 21 * 23 - 3), (30, [255, 255, 255, 0, 0, 0], [255] * 6, 3)])
def test_strips(gpu, d2, mask1, mask2, labels, mode):
    """tests/test_graphcut_model.py's strips: d2 = 0 ties and takes the maximal source side (test_tie_takes_the_maximal_source_side),
    d2 = 30 is test_hand_worked_strip; under COST_COLOR_GRAD the same cuts (test_strips_carry_over)."""
    from test_graphcut_model import strip
    cost, f32 = MODES[mode]
    imgs, corners, masks = strip(d2)
    src = _src(imgs, f32)
    r = check_pair(gpu, src[0], src[1], corners[0], corners[1], masks[0], masks[1], cost_type=cost)
    assert r["flow"] == 8008 * r["flow_scale"] and int(r["labels"].sum()) == labels
    assert masks[0].tolist() == [mask1] and masks[1].tolist() == [mask2]


# ---- the CV_32FC3 value check ------------------------------------------------------------------------------------------------------

def _value_layout():
    """Three overlapping 16 x 20 tiles in a row and a fourth that overlaps none of them."""
    rng = np.random.default_rng(77)
    imgs = [rng.integers(0, 256, (16, 20, 3)).astype(np.float32) for _ in range(4)]
    corners = [(0, 0), (10, 2), (20, 4), (200, 200)]
    masks = [np.full((16, 20), 255, np.uint8) for _ in range(4)]
    return imgs, corners, masks


@pytest.mark.parametrize("cost", [COLOR, GRAD])
@pytest.mark.parametrize("value", BAD_VALUES, ids=["nan", "inf", "-inf", "-1", "256", "0.5", "254.5", "above_255", "denormal"])
def test_value_check(gpu, value, cost):
    """One bad CV_32FC3 value - at the first element or at the last one of the last row; in tile 0, the middle tile, the last tile of the
    three that overlap, or the tile that overlaps nothing; through find() or the pair entry; on host or device mats - is refused with
    ISX_ERR_UNSUPPORTED before any mask is written."""
    imgs, corners, masks = _value_layout()
    fdr = gpu.GraphCutSeamFinder(cost_type=cost)
    for place in ((0, 0, 0), (15, 19, 2)):
        for tile in range(4):
            bad = [a.copy() for a in imgs]
            bad[tile][place] = value
            for where in ("host", "device"):
                n = 4 if tile == 3 else 3
                src = bad[:n] if where == "host" else [_dev(a) for a in bad[:n]]
                m = [x.copy() for x in masks[:n]] if where == "host" else [_dev(x) for x in masks[:n]]
                with pytest.raises(gpu.IsxError) as e:
                    fdr.find(src, corners[:n], m)
                assert e.value.code == 6, (place, tile, where)
                assert all(np.array_equal(_np(a), b) for a, b in zip(m, masks)), (place, tile, where)
                other = 1 if tile == 0 else 0                                # the pair entry: the bad tile second, or first for tile 0
                i, j = (tile, other) if tile == 0 else (other, tile)
                with pytest.raises(gpu.IsxError) as e:
                    fdr.find_pair(src[i], src[j], corners[i], corners[j], m[i], m[j], certificate=(where == "host"))
                assert e.value.code == 6, (place, tile, where, "pair")
                assert all(np.array_equal(_np(a), b) for a, b in zip(m, masks)), (place, tile, where, "pair")


@pytest.mark.parametrize("cost", [COLOR, GRAD])
def test_minus_zero_is_accepted(gpu, cost):
    """-0.0 is an integer in [0, 255]: wherever a 0 stood it gives the masks of +0.0, the model's."""
    for name in ("serp_0", "step_inv"):
        imgs, corners, masks = GC.small_case(name)
        want = solved(name, cost)[3]
        src = _f32(imgs)
        neg = [np.where(a == 0, np.float32(-0.0), a).astype(np.float32) for a in src]
        assert all(np.signbit(a).any() and np.array_equal(a, b) for a, b in zip(neg, src))
        for s in (src, neg):
            m = [x.copy() for x in masks]
            gpu.GraphCutSeamFinder(cost_type=cost).find(s, corners, m)
            assert np.array_equal(m[0], want[0]) and np.array_equal(m[1], want[1])
        dm = [_dev(x) for x in masks]
        gpu.GraphCutSeamFinder(cost_type=cost).find([_dev(a) for a in neg], corners, dm)
        assert np.array_equal(_np(dm[0]), want[0]) and np.array_equal(_np(dm[1]), want[1])


def _nan_in_the_pitch_gap(g):
    """NaN in every float of the lead before and the pad after each row of a guarded CV_32FC3 view, then a fresh snapshot."""
    h = g.shape[0]
    nan = np.frombuffer(np.float32(np.nan).tobytes(), np.uint8)
    fill = np.zeros(g.nbytes, bool)
    pat = np.zeros(g.nbytes, np.uint8)
    for r in range(h):
        start = g.first + (guarded.ROWS_ABOVE + r) * g.pitch
        for a, b in ((start, start + g.lead), (start + g.lead + g.row_bytes, start + g.pitch)):
            n = (b - a) // 4 * 4
            fill[a:a + n] = True
            pat[a:a + n] = np.tile(nan, n // 4)
    assert fill.sum() >= 8 * 4 * h
    if g.where == "host":
        g.buf[fill] = pat[fill]
    else:
        import torch
        buf = g.buf.cpu().numpy()
        buf[fill] = pat[fill]
        g.buf.copy_(torch.from_numpy(buf))
    return g.snapshot()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("cost", [COLOR, GRAD])
def test_nan_in_the_pitch_gap_is_not_read(gpu, cost, where):
    """The value check, the build kernels and the Sobel's three row pointers stay inside the view: NaN before and after every row of
    each image changes nothing, and no byte of the images' buffers is written."""
    name = "xramp_yramp"
    imgs, corners, masks = GC.small_case(name)
    want = solved(name, cost)[3]
    g_src = [_nan_in_the_pitch_gap(guarded.guarded_like(a, where, "odd", 40 + k)) for k, a in enumerate(_f32(imgs))]
    g_mk = [guarded.guarded_like(m, where, "odd", 50 + k) for k, m in enumerate(masks)]
    gpu.GraphCutSeamFinder(cost_type=cost).find([g.view for g in g_src], corners, [g.view for g in g_mk])
    assert np.array_equal(g_mk[0].get(), want[0]) and np.array_equal(g_mk[1].get(), want[1])
    for g in g_mk:
        g.check()
    for g in g_src:
        g.check(guarded.NOTHING)
    m = [x.copy() for x in masks]
    r = check_pair(gpu, g_src[0].view, g_src[1].view, corners[0], corners[1], m[0], m[1], cost_type=cost) if where == "host" else None
    assert r is None or r["flow"] == KNOWN[(name, cost)][0]


def test_grid_limit_refusal(gpu):
    """COST_COLOR_GRAD on a padded grid of 8192 x 8193 nodes, one row past 2^26: ISX_ERR_UNSUPPORTED naming the limit, before anything is
    staged (the 800 MB image is np.zeros and never touched) or written - through the pair entry, and through find() where only the
    last of three pairs is too large and the first would have cut.  The accepted side of the limit is not run: a 3.2 GB graph."""
    big = np.zeros((8172, 8173, 3), np.float32)
    mb = [np.zeros((8172, 8173), np.uint8) for _ in range(2)]
    for m in mb:
        m[:12, :12] = 255
    fdr = gpu.GraphCutSeamFinder(cost_type=GRAD)
    with pytest.raises(gpu.IsxError) as e:
        fdr.find_pair(big, big, (5, 7), (5, 7), mb[0], mb[1])
    assert e.value.code == 6 and "2^26" in str(e.value) and "8192 x 8193" in str(e.value)
    assert all(int(np.count_nonzero(m)) == 144 and (m[:12, :12] == 255).all() for m in mb)
    # three tiles: (0, 1) overlaps by 12 x 12 and would clear mask bytes, (0, 2) likewise, (1, 2) is too large
    small = np.random.default_rng(3).integers(0, 256, (30, 40, 3)).astype(np.float32)
    ms = np.full((30, 40), 255, np.uint8)
    with pytest.raises(gpu.IsxError) as e:
        fdr.find([small, big, big], [(1000 - 28, 1000 - 18), (1000, 1000), (1000, 1000)], [ms, mb[0], mb[1]])
    assert e.value.code == 6 and "2^26" in str(e.value)
    assert (ms == 255).all() and all(int(np.count_nonzero(m)) == 144 and (m[:12, :12] == 255).all() for m in mb)
    # the limit is COST_COLOR_GRAD's alone, and a refusal leaves the finder usable
    ok = fdr.find_pair(small, small, (0, 0), (12, 9), ms.copy(), ms.copy())
    assert (ok["rows"], ok["cols"]) == (41, 48) and ok["flow"] > 0
