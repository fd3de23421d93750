"""Known answers for the NumPy model of GraphCutSeamFinder(COST_COLOR_GRAD) (tests/helpers/graphcut_grad_np.py), the specification of
isx_graphcut_seam_find with ISX_GC_COST_COLOR_GRAD: the squared Sobel norms against a per-pixel loop, the Q23 graph against
setGraphWeightsColorGrad written as OpenCV's loops, two worked capacities, constant tiles (COST_COLOR's graph shifted left by 23, with the
hand-worked strips of tests/test_graphcut_model.py), the model's own max-flow against scipy's and networkx's, and recorded flows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import graphcut_grad_np as GG  # noqa: E402
from helpers import graphcut_np as G  # noqa: E402
from test_graphcut_model import graph_loops, strip  # noqa: E402


def layout(n, seed):
    """The layout() of tests/test_gpu_graphcut_seam.py (that module is GPU-only)."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(40, 90)), int(rng.integers(30, 70))) for _ in range(n)]
    corners = [(int(rng.integers(-30, 30)), int(rng.integers(-20, 20))) for _ in range(n)]
    imgs, masks = [], []
    for w, h in sizes:
        base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3))
        img = np.kron(base, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(0, 12, (h, w, 3))
        imgs.append(np.clip(img, 0, 255).astype(np.uint8))
        m = np.full((h, w), 255, np.uint8)
        for _ in range(3):
            y, x = int(rng.integers(0, h - 4)), int(rng.integers(0, w - 4))
            m[y:y + int(rng.integers(2, 10)), x:x + int(rng.integers(2, 10))] = 0
        masks.append(m)
    return corners, imgs, masks


def pairs_of(n, seed, cost_type=GG.COST_COLOR_GRAD):
    """[(i, j, graph, flow, certificate)] of find() on layout(n, seed), and the final masks."""
    corners, imgs, masks = layout(n, seed)
    seen = []
    out = GG.find(imgs, corners, [m.copy() for m in masks], cost_type, per_pair=lambda *a: seen.append(a))
    return seen, out


def r101(i, n):
    if n == 1:
        return 0
    return -i if i < 0 else 2 * (n - 1) - i if i >= n else i


def sobel_loops(img):
    """Sobel(src, CV_32F, 1, 0) / (0, 1), 3 x 3, BORDER_REFLECT_101, then normL2 of the Point3f, pixel by pixel in float32 as OpenCV."""
    h, w, _ = img.shape
    a = img.astype(np.float32)
    dx, dy = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    kd, ks = (-1, 0, 1), (1, 2, 1)
    for y in range(h):
        for x in range(w):
            for c in range(3):
                sx = sy = np.float32(0)
                for j in range(3):
                    for i in range(3):
                        v = a[r101(y + j - 1, h), r101(x + i - 1, w), c]
                        sx += np.float32(kd[i] * ks[j]) * v
                        sy += np.float32(ks[i] * kd[j]) * v
                dx[y, x] += sx * sx
                dy[y, x] += sy * sy
    return dx, dy


def grad_loops(img1, img2, mask1, mask2, tl1, tl2, roi):
    """findInPair + setGraphWeightsColorGrad as OpenCV's loops, in float32, weights times 2^23."""
    f = np.float32
    gap = G.GAP
    x0, y0, w, h = roi
    Hp, Wp = h + 2 * gap, w + 2 * gap
    s = [np.zeros((Hp, Wp, 3), f), np.zeros((Hp, Wp, 3), f)]
    k = [np.zeros((Hp, Wp), int), np.zeros((Hp, Wp), int)]
    dx = [np.zeros((Hp, Wp), f), np.zeros((Hp, Wp), f)]
    dy = [np.zeros((Hp, Wp), f), np.zeros((Hp, Wp), f)]
    for t, (img, mask, tl) in enumerate(((img1, mask1, tl1), (img2, mask2, tl2))):
        gx, gy = sobel_loops(img)
        for y in range(-gap, h + gap):
            for x in range(-gap, w + gap):
                yy, xx = y0 - tl[1] + y, x0 - tl[0] + x
                if 0 <= yy < img.shape[0] and 0 <= xx < img.shape[1]:
                    s[t][y + gap, x + gap] = img[yy, xx]
                    k[t][y + gap, x + gap] = mask[yy, xx]
                    dx[t][y + gap, x + gap], dy[t][y + gap, x + gap] = gx[yy, xx], gy[yy, xx]
    right, down = np.zeros((Hp, Wp), np.int64), np.zeros((Hp, Wp), np.int64)

    def norm(y, x):
        d = s[0][y, x] - s[1][y, x]
        return f(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])

    for y in range(Hp):
        for x in range(Wp):
            for (yy, xx, g, out) in ((y, x + 1, dx, right), (y + 1, x, dy, down)):
                if yy < Hp and xx < Wp:
                    grad = f(f(f(f(g[0][y, x] + g[0][yy, xx]) + g[1][y, x]) + g[1][yy, xx]) + f(1))
                    wgt = f(f(f(norm(y, x) + norm(yy, xx)) / grad) + f(1))
                    if not (k[0][y, x] and k[0][yy, xx] and k[1][y, x] and k[1][yy, xx]):
                        wgt = f(wgt + f(1000))
                    q = float(wgt) * 2.0 ** 23
                    assert q == int(q)
                    out[y, x] = int(q)
    return dict(right=right, down=down)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (2, 5), (3, 3), (6, 9)])
def test_sobel_sq_against_a_per_pixel_loop(shape):
    rng = np.random.default_rng(shape[0] * 16 + shape[1])
    img = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
    dx, dy = GG.sobel_sq(img)
    wx, wy = sobel_loops(img)
    assert dx.dtype == np.int64 and dx.shape == shape
    assert np.array_equal(dx, wx.astype(np.int64)) and np.array_equal(dy, wy.astype(np.int64))
    assert np.array_equal(GG.sobel_sq(img.astype(np.float32))[0], dx)
    assert max(dx.max(), dy.max()) <= 3 * 1020 ** 2
    if shape[0] == 1:
        assert not dy.any()
    if shape[1] == 1:
        assert not dx.any()


def test_sobel_sq_reaches_its_bound():
    img = np.zeros((3, 3, 3), np.uint8)
    img[:, 2] = 255
    dx, dy = GG.sobel_sq(img)
    assert dx[1, 1] == 3 * 1020 ** 2 == 3121200 and dy[1, 1] == 0


def test_graph_matches_opencvs_loops():
    rng = np.random.default_rng(5)
    for case in range(6):
        w1, h1, w2, h2 = rng.integers(3, 14, 4)
        tl1 = (int(rng.integers(-5, 5)), int(rng.integers(-5, 5)))
        tl2 = (tl1[0] + int(rng.integers(-w2 + 1, w1)), tl1[1] + int(rng.integers(-h2 + 1, h1)))
        img1 = rng.integers(0, 256, (h1, w1, 3)).astype(np.uint8)
        img2 = rng.integers(0, 256, (h2, w2, 3)).astype(np.uint8)
        if case % 2:                                                       # smooth tiles: small gradients, large quotients
            img1, img2 = (img1 // 32 + 100).astype(np.uint8), (img2 // 32 + 90).astype(np.uint8)
        m1 = np.where(rng.random((h1, w1)) < 0.8, 255, 0).astype(np.uint8)
        m2 = np.where(rng.random((h2, w2)) < 0.8, 255, 0).astype(np.uint8)
        roi = G.overlap_roi(tl1, tl2, (w1, h1), (w2, h2))
        assert roi is not None
        g = GG.pair_graph_grad(img1.astype(np.float32), img2.astype(np.float32), m1, m2, tl1, tl2, roi)
        want = grad_loops(img1, img2, m1, m2, tl1, tl2, roi)
        color = graph_loops(img1.astype(float), img2.astype(float), m1, m2, tl1, tl2, roi)
        assert np.array_equal(g["right"], want["right"]) and np.array_equal(g["down"], want["down"]), case
        assert np.array_equal(g["src"], color["src"] << 23) and np.array_equal(g["snk"], color["snk"] << 23), case
        assert g["right"][:, :-1].min() >= 1 << 23 and g["down"][:-1].min() >= 1 << 23


def test_roi_at_a_tile_corner():
    """Tiles meeting corner to corner: the gap reaches past both tiles, where the gradients read 0, and the tiles' own edges reflect."""
    rng = np.random.default_rng(8)
    img1, img2 = (rng.integers(0, 256, (20, 20, 3)).astype(np.uint8) for _ in range(2))
    m = np.full((20, 20), 255, np.uint8)
    roi = G.overlap_roi((0, 0), (15, 15), (20, 20), (20, 20))
    g = GG.pair_graph_grad(img1, img2, m, m, (0, 0), (15, 15), roi)
    want = grad_loops(img1, img2, m, m, (0, 0), (15, 15), roi)
    assert g["src"].shape == (25, 25)
    assert np.array_equal(g["right"], want["right"]) and np.array_equal(g["down"], want["down"])
    assert g["right"][2, 21] == 1001 << 23                                  # off both tiles


def test_two_worked_capacities():
    """Numerator 1 over grad 3: weight 1.3333334f = 11 184 811 / 2^23; with the penalty 1001.3333f = 8 399 792 640 / 2^23.  (On integer
    tiles every dx_ is a sum of squares of integers, so a grad of 3 itself needs dx_ terms of 1 + 1; the graph cases below use 17.)"""
    f = np.float32
    w = f(f(f(1) / f(3)) + f(1))
    assert w == f(1.3333334) and int(float(w) * 2 ** 23) == 11184811
    wp = f(w + f(1000))
    assert wp == f(1001.3333) and int(float(wp) * 2 ** 23) == 8399792640
    assert GG._q23(np.array([w, wp], f)).tolist() == [11184811, 8399792640]
    # through the graph, 1 x 3 tiles at the same place (grid row 10, columns 10..12)
    img1, img2 = np.zeros((1, 3, 3), np.uint8), np.zeros((1, 3, 3), np.uint8)
    m = np.full((1, 3), 255, np.uint8)
    img1[0, 1] = (4, 4, 4)                                                  # |d|^2 = 48 at pixel 1; dx1 = 0 everywhere (pixels 0 and 2 are equal)
    assert GG.sobel_sq(img1)[0][0].tolist() == [0, 0, 0]
    g = GG.pair_graph_grad(img1, img2, m, m, (0, 0), (0, 0), (0, 0, 3, 1))
    assert g["right"][10, 10] == 49 << 23 and g["right"][10, 9] == 1001 << 23 and g["down"][10, 11] == 1049 << 23
    img2[0, 2, 1] = 1                                                       # image 2's dx at pixel 1: (4 * 1)^2 = 16, at pixels 0 and 2: 0
    assert GG.sobel_sq(img2)[0][0].tolist() == [0, 16, 0]
    g = GG.pair_graph_grad(img1, img2, m, m, (0, 0), (0, 0), (0, 0, 3, 1))
    assert g["right"][10, 10] == int(float(f(f(f(48) / f(17)) + f(1))) * 2 ** 23) == 32074090      # 1 + 48 / 17 = 3.8235295f
    assert g["right"][10, 11] == int(float(f(f(f(49) / f(17)) + f(1))) * 2 ** 23)                  # pixel 2 differs by 1 now


def test_constant_tiles_give_colors_graph_shifted():
    rng = np.random.default_rng(3)
    img1 = np.full((30, 40, 3), 0, np.uint8) + np.array([10, 200, 30], np.uint8)
    img2 = np.full((25, 35, 3), 0, np.uint8) + np.array([12, 190, 37], np.uint8)
    m1 = np.where(rng.random((30, 40)) < 0.9, 255, 0).astype(np.uint8)
    m2 = np.where(rng.random((25, 35)) < 0.9, 255, 0).astype(np.uint8)
    roi = G.overlap_roi((0, 0), (11, 7), (40, 30), (35, 25))
    c = G.pair_graph(img1, img2, m1, m2, (0, 0), (11, 7), roi)
    g = GG.pair_graph_grad(img1, img2, m1, m2, (0, 0), (11, 7), roi)
    for k in ("src", "snk", "right", "down"):
        assert np.array_equal(g[k], c[k] << 23), k


@pytest.mark.parametrize("d2,flow,labels", [(30, 8008, 3), (0, 8008, 21 * 23 - 3)])
def test_strips_carry_over(d2, flow, labels):
    """The strips of tests/test_graphcut_model.py.  d2 = 0: constant tiles, COST_COLOR's graph shifted left by 23, the same tie.  d2 = 30:
    image 2 has gradients around its third pixel, which only cheapen edges inside the roi; every edge of the wall around the source-only
    trio keeps weight 1001 and the wall around the sink-only trio costs more than 8008, so that cut stays the only minimum."""
    src, corners, masks = strip(d2=d2)
    roi = G.overlap_roi(corners[0], corners[1], (6, 1), (6, 1))
    g = GG.pair_graph_grad(src[0], src[1], masks[0], masks[1], corners[0], corners[1], roi)
    c = G.pair_graph(src[0], src[1], masks[0], masks[1], corners[0], corners[1], roi)
    if d2 == 0:
        assert all(np.array_equal(g[k], c[k] << 23) for k in ("src", "snk", "right", "down"))
    f, cert = GG.max_flow(g)
    assert f == flow << 23
    G.check_certificate(g, f, cert["residuals"], cert["labels"])
    assert int(cert["labels"].sum()) == labels
    if d2 == 0:                                                            # the tie: minimal side the trio, maximal all but the sink trio
        assert G.minimal_source_side(g, cert["residuals"]).sum() == 3 and not cert["labels"][10, 13:16].any()
    else:
        assert np.array_equal(G.minimal_source_side(g, cert["residuals"]), cert["labels"])     # unique
    out = GG.find(src, corners, [m.copy() for m in masks])
    if d2 == 0:
        assert out[0].tolist() == [[255] * 6] and out[1].tolist() == [[0, 0, 0, 255, 255, 255]]
    else:
        assert out[0].tolist() == [[255, 255, 255, 0, 0, 0]] and out[1].tolist() == [[255] * 6]


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2)])
def test_own_solver_equals_scipys_dinic_on_color_graphs(n, seed):
    pytest.importorskip("scipy")
    seen, out = pairs_of(n, seed, GG.COST_COLOR)
    corners, imgs, masks = layout(n, seed)
    want = []
    G.find(imgs, corners, [m.copy() for m in masks], per_pair=lambda *a: want.append(a))
    assert len(seen) == len(want) >= 1
    for (i, j, g, f, c), (wi, wj, wg, wf, wc) in zip(seen, want):
        assert (i, j, f) == (wi, wj, wf)
        assert np.array_equal(c["labels"], wc["labels"])
        G.check_certificate(g, f, c["residuals"], c["labels"])


KNOWN = {(2, 1): [((38, 36), 446523952224, 642)],
         (3, 2): [((39, 58), 300014603916, 1281), ((34, 80), 177567344665, 1320), ((56, 37), 391411192364, 700)],
         (2, 9): [((61, 47), 630829360673, 2329)]}


@pytest.mark.parametrize("n,seed", sorted(KNOWN))
def test_known_answers(n, seed):
    seen, _ = pairs_of(n, seed)
    assert [(g["src"].shape, f, int(c["labels"].sum())) for _, _, g, f, c in seen] == KNOWN[(n, seed)]
    for _, _, g, f, c in seen:
        G.check_certificate(g, f, c["residuals"], c["labels"])
        assert max(g["right"].max(), g["down"].max()) >= 1 << 33           # penalty edges: both halves of a word matter


@pytest.mark.parametrize("n,seed", sorted(KNOWN))
def test_own_solver_equals_networkx_preflow_push(n, seed):
    nx = pytest.importorskip("networkx")
    from networkx.algorithms.flow import preflow_push
    seen, _ = pairs_of(n, seed)
    for _, _, g, f, c in seen:
        Hp, Wp = g["src"].shape
        nn = Hp * Wp
        D = nx.DiGraph()
        D.add_nodes_from(range(nn + 2))
        u, v, w = G._edges(g)
        for a, b, cap in zip(u.tolist(), v.tolist(), w.tolist()):
            D.add_edge(a, b, capacity=cap)
            D.add_edge(b, a, capacity=cap)
        for k in np.nonzero(g["src"].ravel())[0].tolist():
            D.add_edge(nn, k, capacity=int(g["src"].ravel()[k]))
        for k in np.nonzero(g["snk"].ravel())[0].tolist():
            D.add_edge(k, nn + 1, capacity=int(g["snk"].ravel()[k]))
        assert preflow_push(D, nn, nn + 1, value_only=True).graph["flow_value"] == f


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3), (2, 9)])
def test_masks_differ_from_cost_colors(n, seed):
    """A COST_COLOR_GRAD that silently ran COST_COLOR would give COST_COLOR's masks: on these layouts every tile's mask differs."""
    pytest.importorskip("scipy")
    corners, imgs, masks = layout(n, seed)
    color = G.find(imgs, corners, [m.copy() for m in masks])
    _, grad = pairs_of(n, seed)
    diff = [int((a != b).sum()) for a, b in zip(grad, color)]
    assert all(d > 0 for d in diff), diff
    assert any((a != b).any() for a, b in zip(grad, masks))


def test_unsupported_values_and_fewer_than_two_images():
    m = [np.full((4, 4), 255, np.uint8)]
    GG.find([np.zeros((4, 4, 3), np.float32)], [(0, 0)], m)
    assert (m[0] == 255).all()
    bad = np.zeros((4, 4, 3), np.float32)
    bad[1, 2, 0] = 0.5
    with pytest.raises(G.Unsupported):
        GG.find([np.zeros((4, 4, 3), np.float32), bad], [(0, 0), (2, 2)], [np.full((4, 4), 255, np.uint8) for _ in range(2)])


def test_entry_declared_and_exported():
    from imagestitch_amd import _lib, seam
    assert "isx_graphcut_seam_find_pair64" in _lib.declared_symbols()
    assert seam.COST_COLOR_GRAD == 1 and seam.GraphCutSeamFinder.FLOW_SHIFT == 23
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "imagestitch_hip.h")) as f:
        assert "int isx_graphcut_seam_find_pair64(" in f.read()
