"""Known answers for the NumPy model of GraphCutSeamFinder(COST_COLOR) (tests/helpers/graphcut_np.py), the specification of
isx_graphcut_seam_find: graph construction against a per-pixel restatement of setGraphWeightsColor, hand-worked cuts, the maximal cut
of a tie, the +1000 penalty, a roi at a tile border, pair order over three tiles, and the reference's own tiles."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import graphcut_np as G  # noqa: E402


def graph_loops(img1, img2, mask1, mask2, tl1, tl2, roi):
    """findInPair + setGraphWeightsColor written as OpenCV's loops (sub-images with a gap, then addTermWeights / addEdges)."""
    gap = G.GAP
    x0, y0, w, h = roi
    Hp, Wp = h + 2 * gap, w + 2 * gap
    s1, s2 = np.zeros((Hp, Wp, 3)), np.zeros((Hp, Wp, 3))
    k1, k2 = np.zeros((Hp, Wp), int), np.zeros((Hp, Wp), int)
    for y in range(-gap, h + gap):
        for x in range(-gap, w + gap):
            for img, mask, tl, s, k in ((img1, mask1, tl1, s1, k1), (img2, mask2, tl2, s2, k2)):
                yy, xx = y0 - tl[1] + y, x0 - tl[0] + x
                if 0 <= yy < img.shape[0] and 0 <= xx < img.shape[1]:
                    s[y + gap, x + gap] = img[yy, xx]
                    k[y + gap, x + gap] = mask[yy, xx]
    src, snk = np.zeros((Hp, Wp), int), np.zeros((Hp, Wp), int)
    right, down = np.zeros((Hp, Wp), int), np.zeros((Hp, Wp), int)
    for y in range(Hp):
        for x in range(Wp):
            a, b = (10000 if k1[y, x] else 0), (10000 if k2[y, x] else 0)
            src[y, x], snk[y, x] = max(a - b, 0), max(b - a, 0)       # GCGraph::addTermWeights keeps the difference
            for (yy, xx, out) in ((y, x + 1, right), (y + 1, x, down)):
                if yy < Hp and xx < Wp:
                    wgt = ((s1[y, x] - s2[y, x]) ** 2).sum() + ((s1[yy, xx] - s2[yy, xx]) ** 2).sum() + 1
                    if not (k1[y, x] and k1[yy, xx] and k2[y, x] and k2[yy, xx]):
                        wgt += 1000
                    out[y, x] = wgt
    return dict(src=src, snk=snk, right=right, down=down)


def strip(d2=0):
    """Two 6 x 1 tiles at x = 0 and x = 3, all-zero images except image 2's third overlap pixel (d2 in its first channel).  The roi is
    the three shared pixels; grid row 10 holds three source-only nodes, the roi, three sink-only nodes; every other edge costs 1001."""
    img1 = np.zeros((1, 6, 3), np.uint8)
    img2 = np.zeros((1, 6, 3), np.uint8)
    img2[0, 2, 0] = d2
    return [img1, img2], [(0, 0), (3, 0)], [np.full((1, 6), 255, np.uint8), np.full((1, 6), 255, np.uint8)]


def test_graph_matches_opencvs_loops():
    rng = np.random.default_rng(5)
    for case in range(6):
        w1, h1, w2, h2 = rng.integers(3, 14, 4)
        tl1 = (int(rng.integers(-5, 5)), int(rng.integers(-5, 5)))
        tl2 = (tl1[0] + int(rng.integers(-w2 + 1, w1)), tl1[1] + int(rng.integers(-h2 + 1, h1)))
        img1 = rng.integers(0, 256, (h1, w1, 3)).astype(np.uint8)
        img2 = rng.integers(0, 256, (h2, w2, 3)).astype(np.uint8)
        m1 = np.where(rng.random((h1, w1)) < 0.8, 255, 0).astype(np.uint8)
        m2 = np.where(rng.random((h2, w2)) < 0.8, 255, 0).astype(np.uint8)
        roi = G.overlap_roi(tl1, tl2, (w1, h1), (w2, h2))
        assert roi is not None
        g = G.pair_graph(img1, img2, m1, m2, tl1, tl2, roi)
        f = G.pair_graph(img1.astype(np.float32), img2.astype(np.float32), m1, m2, tl1, tl2, roi)
        want = graph_loops(img1.astype(float), img2.astype(float), m1, m2, tl1, tl2, roi)
        for k in ("src", "snk", "right", "down"):
            assert np.array_equal(g[k], want[k]), (case, k)
            assert np.array_equal(f[k], want[k]), (case, k)


def test_hand_worked_strip():
    """d2 = 30 makes every edge at the third roi pixel 900 dearer, so walling in the sink-only trio costs 7 * 1001 + 1901 = 8908 and
    walling in the source-only trio (six vertical edges, the left end, the edge into the roi) 8 * 1001 = 8008: that cut is the only
    minimum, the roi falls to the sink side and loses mask 1."""
    pytest.importorskip("scipy")
    src, corners, masks = strip(d2=30)
    roi = G.overlap_roi(corners[0], corners[1], (6, 1), (6, 1))
    assert roi == (3, 0, 3, 1)
    g = G.pair_graph(src[0], src[1], masks[0], masks[1], corners[0], corners[1], roi)
    flow, cert = G.max_flow(g)
    assert flow == 8008
    G.check_certificate(g, flow, cert["residuals"], cert["labels"])
    assert np.array_equal(G.minimal_source_side(g, cert["residuals"]), cert["labels"])     # unique
    assert cert["labels"].sum() == 3 and cert["labels"][10, 7:10].all()
    G.find(src, corners, masks)
    assert masks[0].tolist() == [[255, 255, 255, 0, 0, 0]] and masks[1].tolist() == [[255] * 6]


def test_tie_takes_the_maximal_source_side():
    """With d2 = 0 both walls cost 8008: the minimal source side is the source-only trio, the maximal one everything but the sink-only
    trio.  The model takes the maximal one: the roi is source side and mask 2 loses it."""
    pytest.importorskip("scipy")
    src, corners, masks = strip(d2=0)
    g = G.pair_graph(src[0], src[1], masks[0], masks[1], corners[0], corners[1], (3, 0, 3, 1))
    flow, cert = G.max_flow(g)
    assert flow == 8008
    assert G.cut_capacity(g, cert["labels"]) == G.cut_capacity(g, G.minimal_source_side(g, cert["residuals"])) == 8008
    assert G.minimal_source_side(g, cert["residuals"]).sum() == 3
    assert cert["labels"].sum() == 21 * 23 - 3 and not cert["labels"][10, 13:16].any()
    G.find(src, corners, masks)
    assert masks[0].tolist() == [[255] * 6] and masks[1].tolist() == [[0, 0, 0, 255, 255, 255]]


def test_penalty_where_a_mask_byte_is_zero():
    src, corners, masks = strip()
    g = G.pair_graph(src[0], src[1], masks[0], masks[1], corners[0], corners[1], (3, 0, 3, 1))
    assert g["right"][10, 10] == 1 and g["right"][10, 11] == 1            # inside the roi, both masks set
    assert g["right"][10, 9] == 1001 and g["right"][10, 12] == 1001       # one end lacks a mask
    assert g["down"][10, 11] == 1001 and g["right"][0, 0] == 1001         # off the tiles
    masks[1][0, 1] = 0                                                     # roi pixel 1 loses mask 2
    g = G.pair_graph(src[0], src[1], masks[0], masks[1], corners[0], corners[1], (3, 0, 3, 1))
    assert g["right"][10, 10] == 1001 and g["right"][10, 11] == 1001
    assert g["src"][10, 11] == 10000 and g["snk"][10, 11] == 0             # mask 1 only: a source link


def test_a_graph_without_source_or_sink_terminals():
    """One mask empty: the other tile's cells are all of one terminal kind, or - both masks covering the same cells - there is no terminal
    at all.  The flow is 0, the maximal source side is every node that cannot reach a sink link, and find() writes accordingly."""
    pytest.importorskip("scipy")
    img = np.full((12, 14, 3), 50, np.uint8)
    full, empty = np.full((12, 14), 255, np.uint8), np.zeros((12, 14), np.uint8)
    roi = G.overlap_roi((0, 0), (0, 0), (14, 12), (14, 12))
    for m1, m2, src_side in ((full, empty, True), (empty, full, False), (full, full, True), (empty, empty, True)):
        g = G.pair_graph(img, img, m1, m2, (0, 0), (0, 0), roi)
        assert bool(g["src"].any()) == bool(m1.any() and not m2.any()) and bool(g["snk"].any()) == bool(m2.any() and not m1.any())
        flow, cert = G.max_flow(g)
        assert flow == 0
        G.check_certificate(g, flow, cert["residuals"], cert["labels"])
        assert (cert["labels"] == (1 if src_side else 0)).all()              # no sink link anywhere: every node is on the source side
        a, b = m1.copy(), m2.copy()
        G.find([img, img], [(0, 0), (0, 0)], [a, b])
        # source side and mask 1 set -> mask 2 cleared; otherwise mask 2 set -> mask 1 cleared
        assert np.array_equal(a, m1) and np.array_equal(b, empty if (src_side and m1.any()) else m2)


def test_roi_at_a_tile_border():
    """Tiles meeting corner to corner: the gap reaches past both tiles, where nodes read image 0 and mask 0."""
    img1 = np.full((20, 20, 3), 7, np.uint8)
    img2 = np.full((20, 20, 3), 9, np.uint8)
    m = np.full((20, 20), 255, np.uint8)
    roi = G.overlap_roi((0, 0), (15, 15), (20, 20), (20, 20))
    assert roi == (15, 15, 5, 5)
    g = G.pair_graph(img1, img2, m, m, (0, 0), (15, 15), roi)
    assert g["src"].shape == (25, 25)
    assert (g["src"] > 0).sum() == 15 * 15 - 25 and g["src"][:15, :15].sum() == 200 * 10000
    assert (g["snk"] > 0).sum() == 15 * 15 - 25 and g["snk"][10:, 10:].sum() == 200 * 10000
    assert g["right"][12, 12] == 2 * 12 + 1                                  # (7-9)^2 * 3 twice, + 1
    assert g["right"][20, 20] == 9 * 9 * 3 * 2 + 1 + 1000                    # image 2 only
    assert g["right"][2, 2] == 7 * 7 * 3 * 2 + 1 + 1000                      # image 1 only
    assert g["right"][2, 20] == 1 + 1000                                     # off both tiles
    want = graph_loops(img1.astype(float), img2.astype(float), m, m, (0, 0), (15, 15), roi)
    for k in ("src", "snk", "right", "down"):
        assert np.array_equal(g[k], want[k])


def three_tiles():
    """Tiles 0 and 1 show one scene 10 columns apart, except that tile 1 is noise off its columns 8-9 (scene columns 18-19): pair (0, 1)
    cuts there and clears mask 0 right of it - inside tile 2's overlap with tile 0, which pair (0, 2) then reads."""
    rng = np.random.default_rng(11)
    scene = rng.integers(0, 256, (24, 60, 3)).astype(np.uint8)
    imgs = [scene[:, :30].copy(), rng.integers(0, 256, (24, 30, 3)).astype(np.uint8), scene[4:28, 12:42].copy()]
    imgs[1][:, 8:10] = scene[:, 18:20]
    imgs[2] = np.pad(scene, ((0, 8), (0, 0), (0, 0)))[4:28, 12:42].copy()
    corners = [(0, 0), (10, 0), (12, 4)]
    masks = [np.full((24, 30), 255, np.uint8) for _ in range(3)]
    masks[2][5:9, 3:7] = 0
    return imgs, corners, masks


def test_three_tiles_pairs_see_earlier_cuts():
    pytest.importorskip("scipy")
    imgs, corners, masks = three_tiles()
    seen = []
    out = G.find(imgs, corners, [m.copy() for m in masks], per_pair=lambda i, j, g, f, c: seen.append((i, j)))
    assert seen == [(0, 1), (0, 2), (1, 2)]
    # by hand: pair (0, 1), then (0, 2) on the edited masks, then (1, 2)
    ms = [m.copy() for m in masks]
    sizes = [(30, 24)] * 3
    for i, j in ((0, 1), (0, 2), (1, 2)):
        roi = G.overlap_roi(corners[i], corners[j], sizes[i], sizes[j])
        g = G.pair_graph(imgs[i], imgs[j], ms[i], ms[j], corners[i], corners[j], roi)
        _, cert = G.max_flow(g)
        G.write_back(cert["labels"], ms[i], ms[j], corners[i], corners[j], roi)
    assert all(np.array_equal(a, b) for a, b in zip(out, ms))
    # pair (0, 1) cleared mask 0 inside pair (0, 2)'s roi, so (0, 2) built another graph than it would on the unedited masks
    roi01 = G.overlap_roi(corners[0], corners[1], sizes[0], sizes[1])
    m0, m1 = masks[0].copy(), masks[1].copy()
    G.write_back(G.max_flow(G.pair_graph(imgs[0], imgs[1], m0, m1, corners[0], corners[1], roi01))[1]["labels"], m0, m1, corners[0], corners[1], roi01)
    assert (m0[4:, 12:] == 0).any() and (m0[:, :19] == 255).all()
    roi = G.overlap_roi(corners[0], corners[2], sizes[0], sizes[2])
    g0 = G.pair_graph(imgs[0], imgs[2], masks[0], masks[2], corners[0], corners[2], roi)
    g1 = G.pair_graph(imgs[0], imgs[2], m0, masks[2], corners[0], corners[2], roi)
    assert not np.array_equal(g0["src"], g1["src"])


def test_fewer_than_two_images_and_unsupported_values():
    m = [np.full((4, 4), 255, np.uint8)]
    G.find([np.zeros((4, 4, 3), np.float32)], [(0, 0)], m)
    assert (m[0] == 255).all()
    bad = np.zeros((4, 4, 3), np.float32)
    bad[1, 2, 0] = 0.5
    with pytest.raises(G.Unsupported):
        G.find([bad, np.zeros((4, 4, 3), np.float32)], [(0, 0), (2, 2)], [np.full((4, 4), 255, np.uint8) for _ in range(2)])
    for v in (256.0, -1.0, np.nan):
        bad[1, 2, 0] = v
        with pytest.raises(G.Unsupported):
            G.as_int_image(bad)


def test_reference_tiles_known_answers():
    """The reference's warped tiles with the masks that went into its seam finder (tests/test_ref_artifact.py dpseam_case): roi
    287 x 1097, grid 307 x 1117, maximum flow 211 105, maximal source side 152 666 nodes, minimal 129 793."""
    pytest.importorskip("scipy")
    from test_ref_artifact import dpseam_case
    c = dpseam_case()
    sizes = [(a.shape[1], a.shape[0]) for a in c["images"]]
    roi = G.overlap_roi(c["corners"][0], c["corners"][1], sizes[0], sizes[1])
    assert (roi[2], roi[3]) == (287, 1097)
    g = G.pair_graph(c["images"][0], c["images"][1], c["masks_in"][0], c["masks_in"][1], c["corners"][0], c["corners"][1], roi)
    assert g["src"].shape == (1117, 307)
    flow, cert = G.max_flow(g)
    assert flow == 211105
    G.check_certificate(g, flow, cert["residuals"], cert["labels"])
    assert int(cert["labels"].sum()) == 152666
    assert int(G.minimal_source_side(g, cert["residuals"]).sum()) == 129793


def test_entries_declared_and_exported():
    from imagestitch_amd import _lib
    for name in ("isx_graphcut_seam_find", "isx_graphcut_seam_find_pair", "isx_graphcut_seam_release"):
        assert name in _lib.declared_symbols()
    import imagestitch_amd
    assert imagestitch_amd.GraphCutSeamFinder is imagestitch_amd.seam.GraphCutSeamFinder
