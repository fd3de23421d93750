"""The generator and model halves of the fuzz families tools/fuzz_parity.py has for the entry points merged after round 6 (the plane
projector, GainCompensator::feed, the Voronoi and graph-cut seam finders, COLOR_GRAD and seam_gradients, BlocksGainCompensator, cv::resize with
the scaled mask stage) and of the rigs that go round of tools/fuzz_bundle.py and tools/fuzz_bundle_reproj.py, without a GPU: every shape
class of a family is drawn, every drawn case has the shape its class names - recomputed from the case itself, against the tiling
constants read from the kernels' sources -, and the models stay busy on them: few skips, seams that cut, overlaps that count."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_bundle as FB  # noqa: E402
import fuzz_bundle_reproj as FBR  # noqa: E402
import fuzz_parity as F  # noqa: E402
from helpers import voronoi_np as V  # noqa: E402

FAMILIES = {"plane_warp": F.PLANE_CLASSES, "gain_feed": F.GAIN_CLASSES, "voronoi": F.VORONOI_CLASSES, "graphcut": F.GRAPHCUT_CLASSES,
            "seam_grad": F.SEAM_GRAD_CLASSES, "blocks_gain": F.BLOCKS_GAIN_CLASSES, "resize": F.RESIZE_CLASSES,
            "graphcut_grad": F.GRAPHCUT_GRAD_CLASSES, "bundle_wide": FB.WIDE_CLASSES, "bundle_reproj_wide": FB.WIDE_CLASSES}
GEN_SEEDS, MODEL_SEEDS = range(200), range(5000, 5030)
GCG_MODEL_SEEDS = range(5000, 5010)                                     # graphcut_grad's model is a max-flow on Python ints: a third of the seeds


def _rois(c):
    """overlapRoi of every pair i < j of a case with corners and sizes: {(i, j): (x, y, w, h) or None}"""
    n = len(c["sizes"])
    return {(i, j): F.overlap_roi(c["corners"][i], c["corners"][j], c["sizes"][i], c["sizes"][j]) for i in range(n - 1) for j in range(i + 1, n)}


def test_the_constants_are_the_kernels():
    """What the issue that asked for these families read off the kernels; a constant that moves changes these lists, not the test's point."""
    assert F.VR_WIDTHS == [4095, 4096, 4097, 8192, 8193] and F.VR_HEIGHTS == [31, 32, 33, 64, 65]
    assert F.GC_WIDTHS == [63, 64, 65, 128, 129] and F.GC_HEIGHTS == [31, 32, 33, 48]
    assert F.GF_PAIR_SIZES == [4095, 4096, 4097, 8192, 8193] and F.GF_DIAG_SIZES == [16383, 16384, 16385]
    assert F.GRAD_WIDTHS == [63, 64, 65, 129] and F.GRAD_HEIGHTS == [15, 16, 17, 33]
    assert F.SEAM_GAP == V.GAP == 10
    assert [f.__name__ for f in F.CASES[-9:-4]] == F.NEW_FAMILIES and len(F.CASES) == 28
    assert [f.__name__ for f in F.CASES[-4:]] == ["case_blocks_gain", "case_resize", "case_graphcut_grad", "case_plan_verify"]
    assert F.GCG_MAX_NODES == 4600 and F.GCG_THIRD_TILE == (24, 16)
    assert F.BG_WIDE_ROWS == [4095, 4096, 4097, 4101] and F.BG_APPLY_WIDTHS == [255, 256, 257, 511, 512, 513] and F.BG_APPLY_HEIGHTS == [15, 16, 17]
    assert [F._BG[k] for k in ("BA_PX", "BA_ROWS", "LU_NT", "LU_RB", "LU_PNT")] == [4, 4, 256, 8, 1024] and F.BG_MAX_UNKNOWNS == 250
    assert F.RZ_WAVE_WIDTHS == [255, 256, 257, 511, 512, 513] and F.RZ_ROW_HEIGHTS == [3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33]
    assert [F._RZ[k] for k in ("RZ_PX", "DR_ROWS", "RZ_MAX_ROWS")] == [4, 4, 262140] and F.RZ_MAX_SHAPE == (300, 1100)


def check_plane_warp(c):
    w, h = c["w"], c["h"]
    assert c["src"].shape == ((h, w, 3) if c["cn"] == 3 else (h, w)) and 2 <= w <= 400 and 2 <= h <= 300 and c["cn"] in (1, 3)
    assert c["interp"] in (0, 1) and c["border"] in (0, 1, 2, 4)
    if c["cls"] == "tiny":
        assert w <= 4 and h <= 4
    if c["cls"] == "odd_width":
        assert w % 2 == 1
    if c["cls"] == "with_T":
        assert c["T"] is not None and np.any(c["T"] != 0)
    if c["cls"] == "plain":
        assert c["T"] is None


def _check_tiles(c, lo, hi):
    n = len(c["sizes"])
    assert lo <= n <= hi and len(c["corners"]) == n and len(c["masks"]) == n
    for k in range(n):
        assert c["masks"][k].shape == (c["sizes"][k][1], c["sizes"][k][0]) and c["masks"][k].dtype == np.uint8
        if "imgs" in c:
            assert c["imgs"][k].shape == c["masks"][k].shape + (3,)


def check_gain_feed(c):
    _check_tiles(c, 2, 7)
    assert all(a.dtype == np.uint8 for a in c["imgs"]) and all(np.isin(m, (0, 254, 255)).all() for m in c["masks"])
    rois = _rois(c)
    if c["cls"] == "pair_item_edge":
        assert any(r is not None and r[2] * r[3] in F.GF_PAIR_SIZES for r in rois.values())
    if c["cls"] == "diag_item_edge":
        assert any(m.size in F.GF_DIAG_SIZES for m in c["masks"])
    if c["cls"] == "one_pixel_overlap":
        (i, j), r = next((k, r) for k, r in rois.items() if r is not None and r[2] * r[3] == 1)
        x, y = r[:2]
        assert all(c["masks"][k][y - c["corners"][k][1], x - c["corners"][k][0]] == 255 for k in (i, j))      # and it counts
    if c["cls"] == "disjoint_pair":
        assert any(r is None for r in rois.values())


def check_voronoi(c):
    _check_tiles(c, 2, 4)
    rois = [r for r in _rois(c).values() if r is not None]
    if c["cls"] == "chunk_edge":
        assert any(r[2] + 2 * V.GAP in F.VR_WIDTHS and r[3] <= 8 for r in rois)
    if c["cls"] == "seg_edge":
        assert any(r[3] + 2 * V.GAP in F.VR_HEIGHTS for r in rois)
    if c["cls"] == "thin":
        assert any(r[2] == 1 or r[3] == 1 for r in rois)
    if c["cls"] == "no_unique_rows":                                    # pair (0, 1) runs first, on the masks as drawn
        roi = F.overlap_roi(c["corners"][0], c["corners"][1], c["sizes"][0], c["sizes"][1])
        u1, u2 = V.unique_cells(V.submask(c["masks"][0], c["corners"][0], roi), V.submask(c["masks"][1], c["corners"][1], roi))
        rows = slice(V.GAP, V.GAP + roi[3])
        assert (~(u1[rows] != 0).any(axis=1) & ~(u2[rows] != 0).any(axis=1)).any()


def check_graphcut(c):
    _check_tiles(c, 2, 3)
    assert len({a.dtype for a in c["imgs"]}) == 1 and c["imgs"][0].dtype in (np.uint8, np.float32)
    assert all((a >= 0).all() and (a <= 255).all() and (a == np.floor(a)).all() for a in c["imgs"])
    rois = [r for r in _rois(c).values() if r is not None]
    assert all(r[2] <= 130 and r[3] <= 100 for r in rois)                # the model's max-flow stays small
    if c["cls"] == "tile_edge_w":
        assert any(r[2] + 2 * F.SEAM_GAP in F.GC_WIDTHS for r in rois)
    if c["cls"] == "tile_edge_h":
        assert any(r[3] + 2 * F.SEAM_GAP in F.GC_HEIGHTS for r in rois)
    if c["cls"] == "flat_tie":
        assert c["kind"] == "constant"
    if c["kind"] == "constant":
        assert all((a == a[0, 0]).all() for a in c["imgs"])
    if c["cls"] == "holes_heavy":
        assert all(0.2 < float((m == 0).mean()) < 0.4 for m in c["masks"])


def check_graphcut_grad(c):
    import graphcut_cases
    _check_tiles(c, 2, 3)
    assert all(a.dtype == np.float32 for a in c["imgs"])                 # COST_COLOR_GRAD reads Point3f only
    assert all((a >= 0).all() and (a <= 255).all() and (a == np.floor(a)).all() for a in c["imgs"])
    rois = _rois(c)
    g2 = 2 * F.SEAM_GAP
    first = rois[(0, 1)]
    assert first is not None and (first[2] + g2) * (first[3] + g2) <= F.GCG_MAX_NODES         # the roi cap: the model's max-flow stays below 0.5 s
    if len(c["sizes"]) == 3:
        assert c["sizes"][2][0] <= F.GCG_THIRD_TILE[0] and c["sizes"][2][1] <= F.GCG_THIRD_TILE[1]
    assert sum((r[2] + g2) * (r[3] + g2) for r in rois.values() if r is not None) <= F.GCG_MAX_NODES + 2 * (F.GCG_THIRD_TILE[0] + g2) * (F.GCG_THIRD_TILE[1] + g2)
    if c["cls"] == "tile_edge_w":
        assert first[2] + g2 in F.GC_WIDTHS
    if c["cls"] == "tile_edge_h":
        assert first[3] + g2 in F.GC_HEIGHTS
    assert (c["kind"] == "constant") if c["cls"] == "flat_tie" else (c["cls"] not in ("smooth", "noise", "structured") or c["kind"] == c["cls"])
    if c["kind"] == "constant":
        assert all((a == a[0, 0]).all() for a in c["imgs"])
    assert (c["pattern"] in graphcut_cases.PATTERNS) == (c["kind"] == "structured")
    if c["kind"] == "structured":
        for k, (a, (w, h)) in enumerate(zip(c["imgs"], c["sizes"])):
            assert np.array_equal(a, graphcut_cases.pattern_images(c["pattern"], h, w)[k % 2])
    if c["cls"] == "holes_heavy":
        assert all(0.15 < float((m == 0).mean()) < 0.45 for m in c["masks"] if m.size >= 200)


def check_seam_grad(c):
    if c["cls"] == "find":
        n = len(c["imgs"])
        assert 2 <= n <= 3 and len(c["masks"]) == n and len(c["corners"]) == n
        assert all(a.shape == m.shape + (3,) for a, m in zip(c["imgs"], c["masks"]))
        return
    x, y, w, h = c["rect"]
    ih, iw = c["img"].shape[:2]
    assert c["img"].dtype in (np.uint8, np.float32) and c["img"].shape[2] == 3
    assert x >= 0 and y >= 0 and w >= 1 and h >= 1 and x + w <= iw and y + h <= ih
    if c["cls"] == "tile_edge":
        assert w in F.GRAD_WIDTHS or h in F.GRAD_HEIGHTS
    if c["cls"] == "one_pixel":
        assert (w, h) == (1, 1)
    if c["cls"] == "rect_at_border":
        assert x == 0 or y == 0 or x + w == iw or y + h == ih


def check_blocks_gain(c):
    from helpers import blocks_gain_np as BG
    _check_tiles(c, 1, 4)
    assert all(a.dtype == np.uint8 for a in c["imgs"]) and all(np.isin(m, (0, 254, 255)).all() for m in c["masks"])
    blw, blh = c["blocks"]
    assert blw >= 1 and blh >= 1
    B = sum(nx * ny for nx, ny in (BG.block_grid(w, h, blw, blh)[:2] for w, h in c["sizes"]))
    assert 1 <= B <= F.BG_MAX_UNKNOWNS
    diag, pairs = F.bg_record_items(c["corners"], c["sizes"], blw, blh, F._GF["GF_DIAG_BYTES"], F._GF["GF_PAIR_PIXELS"])
    assert len(diag) == B
    assert 1 <= len(c["apply"]) <= 2
    for index, img in c["apply"]:
        assert 0 <= index < len(c["sizes"]) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.size > 0
    rois = _rois(c)
    if c["cls"] == "plain":
        assert len(c["sizes"]) >= 2 and 6 <= blw and 6 <= blh and any(r is not None for r in rois.values())
    if c["cls"] == "several_items":
        assert 96 <= blw <= 256 and 96 <= blh <= 256 and any(len(b) >= 2 for _, _, b in diag + pairs)       # items per record, by the band formula
    if c["cls"] == "wide_row":
        assert blw >= max(w for w, _ in c["sizes"])
        assert any(w in F.BG_WIDE_ROWS and 1 <= h <= 4 and set(b) == {1} for w, h, b in pairs)        # a band is one row
    if c["cls"] == "one_pixel_blocks":
        assert (blw, blh) == (1, 1) and all(w <= 10 and h <= 8 for w, h in c["sizes"]) and B == sum(w * h for w, h in c["sizes"])
    if c["cls"] == "no_pairs":
        assert all(r is None for r in rois.values()) and pairs == []
    if c["cls"] == "one_pixel_meeting":
        assert len(pairs) == 1 and pairs[0][:2] == (1, 1)
        x, y = rois[(0, 1)][:2]
        assert rois[(0, 1)][2:] == (1, 1) and all(c["masks"][k][y - c["corners"][k][1], x - c["corners"][k][0]] == 255 for k in (0, 1))      # and it counts
    if c["cls"] == "apply_edges":
        for index, img in c["apply"]:
            h, w = img.shape[:2]
            assert (w in F.BG_APPLY_WIDTHS or h in F.BG_APPLY_HEIGHTS) and (w, h) != c["sizes"][index]


def check_resize(c):
    src, (dw, dh) = c["src"], c["dsize"]
    sh, sw = src.shape[:2]
    assert (str(src.dtype), 1 if src.ndim == 2 else src.shape[2]) in F.RZ_TYPES and src.ndim in (2, 3) and c["interp"] in (0, 1)
    assert 1 <= sh <= F.RZ_MAX_SHAPE[0] and 1 <= dh <= F.RZ_MAX_SHAPE[0] and 1 <= sw <= F.RZ_MAX_SHAPE[1] and 1 <= dw <= F.RZ_MAX_SHAPE[1]
    st = c["stage"]
    assert (st is not None) == (src.dtype == np.uint8 and src.ndim == 2)                 # the mask stage rides on every CV_8UC1 case
    if st is not None:
        assert st["element"] in F.RZ_ELEMENTS and st["mode"] in F.RZ_STAGE_MODES
        assert st["warped"].shape == (dh, dw) and st["warped"].dtype == np.uint8 and np.isin(st["warped"], (0, 0x5a, 255)).all()
    if c["cls"] == "wave_edge":
        assert dw in F.RZ_WAVE_WIDTHS
    if c["cls"] == "rows_edge":
        assert dh in F.RZ_ROW_HEIGHTS
    if c["cls"] == "half":
        assert sw == 2 * dw and sh == 2 * dh
    if c["cls"] == "half_one_axis":
        assert (sw == 2 * dw) != (sh == 2 * dh)
    if c["cls"] == "tiny_src":
        assert min(sh, sw) <= 3
    if c["cls"] == "steep":
        for a, b in ((sh, dh), (sw, dw)):
            assert 6 * min(a, b) <= max(a, b) <= 12 * min(a, b)
    if c["cls"] == "specials":
        if src.dtype == np.uint8:
            assert np.isin(src, (0, 255)).all()
        else:
            bits = src.view(np.uint32)
            assert np.isfinite(src).all()
            if src.size >= 10:                                              # every kind: a denormal, a -0.0, FLT_MAX
                assert (((bits & 0x7f800000) == 0) & ((bits & 0x007fffff) != 0)).any() and (bits == 0x80000000).any() and (src == np.float32(3.4028235e38)).any()


# ---- the rigs that go round of tools/fuzz_bundle.py and tools/fuzz_bundle_reproj.py: generators keyed by a seed, models that never skip -------
def _gen_wide(tool):
    def gen(rng):
        c = tool.make_wide_case(int(rng.integers(1 << 30)))
        c["where"] = "host" if c["layout"] == "host" else "device"      # strided mats are device mats
        return c
    return gen


def _model_wide(tool):
    """The model's outputs with the branches of bundle_math.hpp it took on the way (tests/bundle_math_cases.BranchCounter)."""
    def model(c):
        import bundle_math_cases as mc
        with mc.BranchCounter() as b:
            outs = tool.run_model(c)
        return dict(outs=outs, taken=b.taken)
    return model


EXTRA = {"bundle_wide": (_gen_wide(FB), _model_wide(FB)), "bundle_reproj_wide": (_gen_wide(FBR), _model_wide(FBR))}


def _family(family):
    """(gen(rng), model(case)) of a family: tools/fuzz_parity.py's, or EXTRA's"""
    return EXTRA[family] if family in EXTRA else (getattr(F, "gen_" + family), getattr(F, "model_" + family))


def check_bundle_wide(c):
    import bundle_cases as bc
    n0 = c["rig_first"][1] if c["rig_first"] is not None else len(c["sizes"])
    Rs, step = c["rotations"], c["step_deg"]
    assert c["wide"] and c["fault"] == 0 and c["layout"] in FB.LAYOUTS and len(Rs) == n0 and 3 <= n0 <= 9 and 20.0 <= step <= 60.0
    assert 1 <= c["max_iter"] <= 6 or (c["max_iter"] in (40, 1000) and n0 <= 3)
    first = [(i, j) for i, j in c["pairs"] if j < n0]
    assert first == sorted(first) and all(i < j for i, j in first) and len(first) >= n0 - 1
    assert all(min(j - i, n0 - (j - i)) in c["steps"] and bc.axes_apart_deg(Rs[i], Rs[j]) < bc.MAX_AXES_DEG for i, j in first)
    assert all((i, i + 1) in first for i in range(n0 - 1))                                   # the chain is always there
    span = (n0 - 1) * step
    if c["cls"] == "ring":
        assert n0 >= 6 and abs(n0 * step - 360.0) < 1e-9 and (0, n0 - 1) in first            # it closes
    if c["cls"] == "arc":
        assert span <= 300.0
    assert span >= 40.0                                                                      # past what planted_rotations ever draws between two cameras
    rest = len(c["sizes"]) - n0
    assert rest in (0, 2, 3, 4) and c["cameras_in"].shape == (n0 + rest, 16) and c["counts"].shape == (1, len(c["pairs"]))


def check_bundle_reproj_wide(c):
    check_bundle_wide(c)
    assert 0 <= c["refine_flags"] <= 31 and c["max_iter"] != 1000


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_class_is_drawn_and_has_its_shape(family):
    gen, check = _family(family)[0], globals()["check_" + family]
    seen = set()
    for seed in GEN_SEEDS:
        c = gen(np.random.default_rng(seed))
        assert c["cls"] in FAMILIES[family]
        check(c)
        seen.add(c["cls"])
        if "where" in c:
            seen.add(c["where"])
    assert seen >= set(FAMILIES[family]), set(FAMILIES[family]) - seen
    assert seen >= {"host", "device"}                                   # and the ways the mats are handed over


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_models_stay_busy(family):
    """30 cases through gen + model: at most 10 % skips; the seam finders' models change a mask in at least half of the cases that have
    masks (all of them, but for seam_grad's gradient half); at least half of the gain cases count an overlap (an off-diagonal N above 1,
    the value an empty intersection gets), and at least half of the blocks-gain cases have an off-diagonal record with N above 1; at least
    half of the rigs that go round are adjusted (an iteration or more) through a branch of bundle_math.hpp that no narrow rig takes; the resize
    family never skips, and at least half of its up-scaled byte cases (larger in both directions) come out with more than 2 distinct values."""
    if family == "graphcut":
        pytest.importorskip("scipy")
    gen, model = _family(family)
    skips = busy = with_masks = upscaled = 0
    seeds = GCG_MODEL_SEEDS if family == "graphcut_grad" else MODEL_SEEDS
    for seed in seeds:
        c = gen(np.random.default_rng(seed))
        want = model(c)
        if isinstance(want, str):
            assert want == "skip"
            skips += 1
        elif family == "gain_feed":
            N = want["N"]
            busy += bool((N - np.diag(np.diag(N)) > 1).any())
        elif family == "resize":
            assert want["out"].shape[:2] == c["dsize"][::-1] and (want["stage"] is None) == (c["stage"] is None)
            if c["src"].dtype == np.uint8 and c["dsize"][0] > c["src"].shape[1] and c["dsize"][1] > c["src"].shape[0]:
                upscaled += 1
                busy += len(np.unique(want["out"] if want["stage"] is None else want["stage"])) > 2
        elif family == "blocks_gain":
            busy += any(p[2] > 1 for p in want["pairs"])
            if c["cls"] == "no_pairs":                                   # diag and b are the same sums: the quotient is exact
                assert want["pairs"] == [] and np.all(want["gains"] == 1.0)
        elif family in EXTRA:                                            # busy: a branch that no narrow rig takes was taken, and the rig was adjusted
            import bundle_math_cases as mc
            busy += any(want["taken"][k] for k in mc.NARROW_NEVER) and int(want["outs"][2][0, 1]) >= 1
        elif "masks" in c:
            with_masks += 1
            masks = want[0] if family in ("graphcut", "graphcut_grad") else want
            busy += any((a != b).any() for a, b in zip(masks, c["masks"]))
    n = len(seeds)
    print(family, "skips", skips, "busy", busy, "of", with_masks or upscaled or n)
    assert skips * 10 <= n
    if family == "resize":
        assert skips == 0 and upscaled >= 3 and busy * 2 >= upscaled, (skips, busy, upscaled)
        return
    if family in ("gain_feed", "blocks_gain") or family in EXTRA:
        assert busy * 2 >= n, (busy, n)
    elif family != "plane_warp":
        assert with_masks >= (n // 3 if family == "seam_grad" else n - skips) and busy * 2 >= with_masks, (busy, with_masks, n)


def test_graphcut_grads_structured_class_yields_ties():
    """The structured and flat_tie classes are there for graphs whose minimum cuts tie: among the first cases of either class, at least
    half have a first pair whose minimal and maximal source side differ (the model's own max-flow, Python ints)."""
    from helpers import graphcut_grad_np as GG
    from helpers import graphcut_np as GN
    ties = {"structured": 0, "flat_tie": 0}
    seen = {"structured": 0, "flat_tie": 0}
    patterns = set()
    for seed in range(400):
        rng = np.random.default_rng(seed)
        c = F.gen_graphcut_grad(rng)
        if c["cls"] == "structured":
            patterns.add(c["pattern"])
        if c["cls"] not in seen or seen[c["cls"]] == 6 or len(c["sizes"]) != 2:
            continue
        seen[c["cls"]] += 1
        roi = F.overlap_roi(c["corners"][0], c["corners"][1], c["sizes"][0], c["sizes"][1])
        g = GG.pair_graph_grad(c["imgs"][0], c["imgs"][1], c["masks"][0], c["masks"][1], c["corners"][0], c["corners"][1], roi)
        flow, cert = GG.max_flow(g)
        low = GN.minimal_source_side(g, cert["residuals"])
        assert GN.cut_capacity(g, low) == flow
        ties[c["cls"]] += not np.array_equal(low, cert["labels"])
    import graphcut_cases
    print("ties", ties, "of", seen)
    assert seen == {"structured": 6, "flat_tie": 6} and all(2 * ties[k] >= seen[k] for k in seen), (ties, seen)
    assert patterns == set(graphcut_cases.PATTERNS)                      # every pattern is drawn


def test_plan_verify_generator_and_model():
    """Family 28 (case_plan_verify): every class is drawn and every drawn camera is of its class, judged again from K, R and the size; true
    plans and shifted ones are both drawn, every bound in both directions; the model skips at most 10 %, calls no true plan MUST_FLAG and three
    in four MUST_PASS, no moved plan MUST_PASS and nine in ten MUST_FLAG, and leaves at most 10 % of all plans without a claim."""
    from helpers import plan_verify_np as PV
    seen, shifts = set(), set()
    for seed in GEN_SEEDS:
        c = F.gen_plan_verify(np.random.default_rng(seed))
        assert c["cls"] in F.PLAN_VERIFY_CLASSES and F.pv_is_of_class(c), (seed, c["cls"])
        assert (c["w"], c["h"]) in F.PV_SIZES and c["K"].dtype == np.float32 and c["R"].dtype == np.float32
        assert 0.49 <= c["scale"] / float(c["K"][0, 0]) <= 2.01
        assert np.allclose(c["R"] @ c["R"].T, np.eye(3), atol=1e-5)
        assert c["shift"] is None or (c["shift"][0] in range(4) and 1 <= abs(c["shift"][1]) <= 40)
        if c["cls"] == "zero_bound":
            assert min(abs(float(c["K"][0, 2])), abs(float(c["K"][1, 2]))) < 0.61
        seen.add(c["cls"])
        shifts.add(None if c["shift"] is None else (c["shift"][0], int(np.sign(c["shift"][1]))))
    assert seen == set(F.PLAN_VERIFY_CLASSES)
    assert shifts == {None} | set(PV.SHIFTS)
    verdicts = {True: [], False: []}
    skips = 0
    for seed in range(5000, 5240):
        c = F.gen_plan_verify(np.random.default_rng(seed))
        want = F.model_plan_verify(c)
        if isinstance(want, str):
            assert want == "skip"
            skips += 1
            continue
        assert [PV.f2i(e) for e in want["extrema"]] == want["roi"]
        verdicts[c["shift"] is None].append(want["verdict"])
    true, moved = verdicts[True], verdicts[False]
    print("skips", skips, "true", {v: true.count(v) for v in set(true)}, "moved", {v: moved.count(v) for v in set(moved)})
    assert skips * 10 <= 240 and len(true) >= 40 and len(moved) >= 120
    assert PV.MUST_FLAG not in true and true.count(PV.MUST_PASS) * 4 >= len(true) * 3       # (a tile on the back seam has a border pixel within the allowance of it now and then)
    assert PV.MUST_PASS not in moved and moved.count(PV.MUST_FLAG) * 10 >= len(moved) * 9
    assert (true + moved).count(PV.NO_CLAIM) * 10 <= len(true + moved)


def test_homography_large_class_is_drawn_and_the_older_classes_draw_what_they_drew():
    """tools/fuzz_homography.py: a soak's first 200 cases (scheduled(): the classes in turn) hold the `large` class with counts past 300 - the
    most any older class or test reached - up to thousands; it has a generator of its own, so case(seed, cls) of the six older classes
    gives the bytes it gave before (digests taken from the generator as it was)."""
    import hashlib
    import fuzz_homography as FH

    def digest(c):
        h = hashlib.sha256()
        for p, n in c["pairs"]:
            h.update(np.ascontiguousarray(p).tobytes())
            h.update(repr(int(n)).encode())
        h.update(repr((sorted(c["kw"].items()), c["device"], c["wide"], c["spare"])).encode())
        return h.hexdigest()[:16]
    counts = []
    for n in range(200):
        s, cls = FH.scheduled(20261201, n)
        if cls == "large":
            c = FH.case(s, cls)
            (pts, count), = c["pairs"]
            assert count == len(pts) and 400 <= count <= 9000 and c["kw"] == {}
            counts.append(count)
    assert len(counts) >= 28 and min(counts) > 300 and max(counts) > 8192 - 1500 and sum(1 for v in counts if v > 2000) >= 10, counts
    assert FH.CLASSES[:6] == ("tiny", "chunk_edges", "count_limits", "noisy", "degenerate", "multi")
    want = {(1, "tiny"): "a39b4b39d9efe37e", (2, "chunk_edges"): "f57296396d7e14d2", (3, "noisy"): "baca7781bd07449b", (4, "multi"): "d5a8ec2f22e57291",
            (5, "degenerate"): "cc51dd68cdb99d7b"}
    assert {k: digest(FH.case(*k)) for k in want} == want
    assert FH.lm_iters_of(7) == int(np.random.default_rng([7, 0x4C4D]).choice([1, 2, 10]))
