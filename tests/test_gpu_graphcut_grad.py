"""GraphCutSeamFinder(COST_COLOR_GRAD) on the GPU (isx_graphcut_seam_find, isx_graphcut_seam_find_pair64) against the NumPy model of
tests/helpers/graphcut_grad_np.py: masks byte for byte on random 2-, 3- and 4-tile layouts (host, device, pitched and unaligned mats), the
64-bit certificate of every pair's maximum flow and maximal cut checked in NumPy against the model's Q23 graph (which checks every capacity
bit for bit through r + r' = 2 w), the smallest shapes, the reference's tiles, the error paths, COST_COLOR and COST_COLOR_GRAD alternating
on one thread and on two, the C++ mirror and OpenCV adapter, and warp -> convertTo -> graph cut -> dilate & AND -> Feather against the
oracle.  The full 4K pair is not here: tools/time_graphcut_seam.py --cost color_grad runs it."""
import gc
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import graphcut_grad_np as GG  # noqa: E402
from helpers import graphcut_np as G  # noqa: E402
from helpers import guarded  # noqa: E402
from imagestitch_amd import synth  # noqa: E402
from test_graphcut_grad_model import KNOWN, layout  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD = GG.COST_COLOR_GRAD


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _f32(imgs):
    return [a.astype(np.float32) for a in imgs]


@functools.lru_cache(maxsize=None)
def _model(n, seed, cost_type=GRAD):
    corners, imgs, masks = layout(n, seed)
    out = GG.find(imgs, corners, [m.copy() for m in masks], cost_type)
    for m in out:
        m.setflags(write=False)
    return tuple(out)


def model(n, seed, cost_type=GRAD):
    """The model's masks of layout(n, seed): solved once, shared, read-only."""
    return list(_model(n, seed, cost_type))


def check_pair(gpu, img1, img2, tl1, tl2, m1, m2, cost_type=GRAD, fdr=None):
    """find_pair with the 64-bit certificate on host masks m1, m2 (edited in place): the certificate proves a maximum flow and the maximal
    cut of the model's graph, and the masks are the write-back of its labels.  Returns the result, or None without an overlap."""
    sizes = [(a.shape[1], a.shape[0]) for a in (img1, img2)]
    roi = G.overlap_roi(tl1, tl2, sizes[0], sizes[1])
    g = GG.pair_graph(_np(img1), _np(img2), m1, m2, tl1, tl2, roi, cost_type) if roi else None
    w1, w2 = m1.copy(), m2.copy()
    r = (fdr or gpu.GraphCutSeamFinder(cost_type=cost_type)).find_pair(img1, img2, tl1, tl2, m1, m2, certificate=True, wide=True)
    if roi is None:
        assert r["rows"] == 0 and r["flow"] == 0 and np.array_equal(m1, w1) and np.array_equal(m2, w2)
        return None
    assert (r["rows"], r["cols"]) == (roi[3] + 20, roi[2] + 20) and r["residuals"].dtype == np.int64
    assert r["flow_scale"] == (1 << 23 if cost_type == GRAD else 1)
    G.check_certificate(g, r["flow"], r["residuals"], r["labels"])
    G.write_back(r["labels"], w1, w2, tl1, tl2, roi)
    assert np.array_equal(m1, w1) and np.array_equal(m2, w2)
    assert r["rounds"] >= 0 and r["launches"] > 0
    r["graph"] = g
    return r


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3)])
@pytest.mark.parametrize("where", ["host", "device", "host_view", "device_view"])
def test_model_parity(gpu, n, seed, where):
    corners, imgs, masks = layout(n, seed)
    want = model(n, seed)
    assert any((w != m).any() for w, m in zip(want, masks))          # the seams cut something
    src = _f32(imgs)
    if where in ("host", "device"):
        src_v = [_dev(a) for a in src] if where == "device" else [a.copy() for a in src]
        mk_v = [_dev(m) for m in masks] if where == "device" else [m.copy() for m in masks]
    else:
        g_src = [guarded.guarded_like(a, where.split("_")[0], "odd", 100 * seed + k) for k, a in enumerate(src)]
        g_mk = [guarded.guarded_like(a, where.split("_")[0], "odd", 100 * (seed + 1) + k) for k, a in enumerate(masks)]
        src_v, mk_v = [g.view for g in g_src], [g.view for g in g_mk]
    gpu.GraphCutSeamFinder(cost_type=GRAD).find(src_v, corners, mk_v)
    for k in range(n):
        assert np.array_equal(_np(mk_v[k]), want[k]), (k, int((_np(mk_v[k]) != want[k]).sum()))
    if where not in ("host", "device"):
        for g in g_mk:
            g.check()                                                # nothing around a mask was written
        for g in g_src:
            g.check(guarded.NOTHING)                                 # ... and the images are inputs


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3), (2, 9)])
def test_masks_are_not_cost_colors(gpu, n, seed):
    """A COST_COLOR_GRAD that ran COST_COLOR would give these masks instead."""
    pytest.importorskip("scipy")
    corners, imgs, masks = layout(n, seed)
    color = G.find(imgs, corners, [m.copy() for m in masks])
    got = [m.copy() for m in masks]
    gpu.GraphCutSeamFinder(cost_type=GRAD).find(_f32(imgs), corners, got)
    assert all((a != b).any() for a, b in zip(got, color))
    assert all(np.array_equal(a, b) for a, b in zip(got, model(n, seed)))


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3), (2, 9)])
def test_certificate_of_every_pair(gpu, n, seed):
    """The one-pair form on every overlapping pair in find()'s order: its 64-bit certificate proves a maximum flow and the maximal
    minimum cut of the model's Q23 graph (NumPy only), and its masks continue the sequence find() produces."""
    corners, imgs, masks = layout(n, seed)
    src = _f32(imgs)
    ms = [m.copy() for m in masks]
    fdr = gpu.GraphCutSeamFinder(cost_type=GRAD)
    seen = []
    for i in range(n - 1):
        for j in range(i + 1, n):
            r = check_pair(gpu, src[i], src[j], corners[i], corners[j], ms[i], ms[j], fdr=fdr)
            if r is not None:
                seen.append(((r["rows"], r["cols"]), r["flow"], int(r["labels"].sum())))
                assert int(r["residuals"].max()) >= 1 << 33          # both halves of a word matter
    assert len(seen) >= 1
    if (n, seed) in KNOWN:
        assert seen == KNOWN[(n, seed)]
    assert all(np.array_equal(a, b) for a, b in zip(ms, model(n, seed)))
    got = [m.copy() for m in masks]
    fdr.find(src, corners, got)
    assert all(np.array_equal(a, b) for a, b in zip(got, ms))


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2)])
def test_cost_color_through_the_64_bit_entry(gpu, n, seed):
    """COST_COLOR through isx_graphcut_seam_find_pair64 against isx_graphcut_seam_find_pair: both certificates prove a maximum flow of
    the model's graph, with the same flow, labels and masks.  The residuals themselves are not compared: a maximum flow is not unique,
    and which one the push-relabel sweeps reach depends on whether a node reads a neighbour's edge word before or after that neighbour's
    push in the same launch - two calls of the int32 entry differ in their residuals just as the two entries do (printed below; on an
    MI355X: on layout(2, 1) 745 of 8 208 words differ between two int32 calls, 734 between the entries)."""
    corners, imgs, masks = layout(n, seed)
    a, b, c = ([m.copy() for m in masks] for _ in range(3))
    fdr = gpu.GraphCutSeamFinder()
    for i in range(n - 1):
        for j in range(i + 1, n):
            roi = G.overlap_roi(corners[i], corners[j], *[(x.shape[1], x.shape[0]) for x in (imgs[i], imgs[j])])
            g = G.pair_graph(imgs[i], imgs[j], a[i], a[j], corners[i], corners[j], roi) if roi else None
            r32 = fdr.find_pair(imgs[i], imgs[j], corners[i], corners[j], a[i], a[j], certificate=True)
            again = fdr.find_pair(imgs[i], imgs[j], corners[i], corners[j], c[i], c[j], certificate=True)
            r64 = check_pair(gpu, imgs[i], imgs[j], corners[i], corners[j], b[i], b[j], cost_type=GG.COST_COLOR, fdr=fdr)
            if r64 is None:
                continue
            assert r32["residuals"].dtype == np.int32 and r32["flow_scale"] == 1
            G.check_certificate(g, r32["flow"], r32["residuals"], r32["labels"])
            print("pair", i, j, "residual words", r32["residuals"].size, "differing: int32 twice", int((r32["residuals"] != again["residuals"]).sum()),
                  "int32 / int64", int((r32["residuals"] != r64["residuals"]).sum()))
            assert int(r64["residuals"].max()) < 1 << 31
            assert r64["flow"] == r32["flow"] and np.array_equal(r64["labels"], r32["labels"])
            assert np.array_equal(a[i], b[i]) and np.array_equal(a[j], b[j])


def _tile(rng, h, w):
    return rng.integers(0, 256, (h, w, 3)).astype(np.float32), np.full((h, w), 255, np.uint8)


SMALL = {
    "one_row": ((1, 9), (0, 0), (1, 9), (8, 0)),                     # (rows, cols), corner, twice: the tiles share one pixel
    "one_column": ((9, 1), (0, 0), (9, 1), (0, 8)),
    "2x2": ((2, 2), (0, 0), (2, 2), (1, 1)),
    "3x3": ((3, 3), (0, 0), (3, 3), (2, 2)),
    "one_pixel_tiles": ((1, 1), (5, 5), (1, 1), (5, 5)),
    "inside_another": ((40, 50), (0, 0), (7, 9), (20, 13)),
    "gap_past_both_tiles": ((12, 12), (0, 0), (12, 12), (9, 9)),     # roi 3 x 3 at both tiles' corners: the gap leaves both
    "wide_and_flat": ((3, 150), (0, 0), (3, 150), (10, 1)),          # more than two launch blocks and BFS tiles across
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_smallest_shapes(gpu, name):
    """Tiles whose reflection degenerates (1 row, 1 column, 2 x 2, 3 x 3 sharing one pixel: a 21 x 21 grid), a tile wholly inside
    another, a roi whose gap reaches past both tiles: certificate and masks against the model; then find() on device mats."""
    (h1, w1), tl1, (h2, w2), tl2 = SMALL[name]
    rng = np.random.default_rng(len(name) + h1 * w2)
    (i1, m1), (i2, m2) = _tile(rng, h1, w1), _tile(rng, h2, w2)
    if min(h1, w1) > 4:
        m1[1:3, 2:4] = 0
    want = GG.find([i1, i2], [tl1, tl2], [m1.copy(), m2.copy()])
    a, b = m1.copy(), m2.copy()
    r = check_pair(gpu, i1, i2, tl1, tl2, a, b)
    if name in ("one_row", "one_column", "2x2", "3x3", "one_pixel_tiles"):
        assert (r["rows"], r["cols"]) == (21, 21)
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1])
    dm = [_dev(m1), _dev(m2)]
    gpu.GraphCutSeamFinder(cost_type=GRAD).find([_dev(i1), _dev(i2)], [tl1, tl2], dm)
    assert np.array_equal(_np(dm[0]), want[0]) and np.array_equal(_np(dm[1]), want[1])


def test_reference_tiles(gpu):
    """The reference's warped tiles (CV_32FC3) with the masks that went into its seam finder, grid 1117 x 307: the certificate against
    the model's Q23 graph, flow 186 520 130 676, maximal source side 13 640 nodes, 877 481 and 1 192 318 mask bytes left (solved once on
    a CPU with networkx's preflow_push, 86 s; here the certificate proves them); the same through find() on device mats."""
    from test_ref_artifact import dpseam_case
    c = dpseam_case()
    m = [x.copy() for x in c["masks_in"]]
    r = check_pair(gpu, c["images"][0], c["images"][1], c["corners"][0], c["corners"][1], m[0], m[1])
    assert (r["rows"], r["cols"]) == (1117, 307)
    assert r["flow"] == 186520130676 and int(r["labels"].sum()) == 13640
    assert [int(np.count_nonzero(x)) for x in m] == [877481, 1192318]
    md = [_dev(x) for x in c["masks_in"]]
    gpu.GraphCutSeamFinder(cost_type=GRAD).find([_dev(a) for a in c["images"]], c["corners"], md)
    assert np.array_equal(_np(md[0]), m[0]) and np.array_equal(_np(md[1]), m[1])


def test_errors_leave_the_masks_untouched(gpu):
    import ctypes as C
    import torch
    from imagestitch_amd import _lib
    from imagestitch_amd._lib import as_mat
    corners, imgs, masks = layout(3, 2)
    f32 = _f32(imgs)
    bad = [a.copy() for a in f32]
    bad[2][5, 7, 1] += 0.5                                          # read by the last pair only: still refused before the first writes
    fdr = gpu.GraphCutSeamFinder(cost_type=GRAD)
    for where in ("host", "device"):
        m = [x.copy() for x in masks] if where == "host" else [_dev(x) for x in masks]
        with pytest.raises(gpu.IsxError) as e:
            fdr.find(bad if where == "host" else [_dev(a) for a in bad], corners, m)
        assert e.value.code == 6
        assert all(np.array_equal(_np(a), b) for a, b in zip(m, masks))
    # byte tiles: OpenCV's finder reads Point3f only
    m = [x.copy() for x in masks]
    with pytest.raises(gpu.IsxError) as e:
        fdr.find_pair(imgs[0], imgs[1], corners[0], corners[1], m[0], m[1], certificate=True)
    assert e.value.code == 6 and all(np.array_equal(a, b) for a, b in zip(m, masks))
    # the int32 certificate cannot hold Q23 residuals: ISX_ERR_INVALID, naming the 64-bit entry; without a certificate the entry runs
    lib = _lib.load()
    m1, m2, k1, k2 = as_mat(f32[0]), as_mat(f32[1]), as_mat(m[0]), as_mat(m[1])
    c4 = (C.c_int * 4)(*corners[0], *corners[1])
    res, lab = np.zeros((100 * 100, 6), np.int32), np.zeros(100 * 100, np.uint8)
    flow, info = C.c_longlong(0), (C.c_int * 4)()
    rc = lib.isx_graphcut_seam_find_pair(C.byref(m1), C.byref(m2), c4, C.byref(k1), C.byref(k2), GRAD, C.byref(flow),
                                         res.ctypes.data_as(C.POINTER(C.c_int)), lab.ctypes.data_as(C.POINTER(C.c_ubyte)), 100 * 100, info, 0, None)
    assert rc == 1 and b"isx_graphcut_seam_find_pair64" in lib.isx_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(m, masks)) and not res.any()
    rc = lib.isx_graphcut_seam_find_pair(C.byref(m1), C.byref(m2), c4, C.byref(k1), C.byref(k2), GRAD, C.byref(flow), None, None, 0, info, 0, None)
    assert rc == 0 and flow.value == KNOWN[(3, 2)][0][1] and (info[0], info[1]) == KNOWN[(3, 2)][0][0]
    # cert_nodes too small: ISX_ERR_SIZE, nothing written
    m = [x.copy() for x in masks]
    k1, k2 = as_mat(m[0]), as_mat(m[1])
    res64 = np.zeros((100 * 100, 6), np.int64)
    n = KNOWN[(3, 2)][0][0][0] * KNOWN[(3, 2)][0][0][1]
    rc = lib.isx_graphcut_seam_find_pair64(C.byref(m1), C.byref(m2), c4, C.byref(k1), C.byref(k2), GRAD, C.byref(flow),
                                           res64.ctypes.data_as(C.POINTER(C.c_longlong)), lab.ctypes.data_as(C.POINTER(C.c_ubyte)), n - 1, info, 0, None)
    assert rc == 7 and not res64.any() and all(np.array_equal(a, b) for a, b in zip(m, masks))
    # a capturing stream: ISX_ERR_STATE before anything is enqueued
    dm, di = [_dev(x) for x in masks], [_dev(a) for a in f32]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    # a CUDAGraph that a dead reference cycle still holds (a test frame kept by its own pytest.raises info) must not be freed by a collection
    # that happens to run inside this capture: its destructor synchronises the device, which a capturing stream turns into an abort
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        with pytest.raises(gpu.IsxError) as e:
            gpu.GraphCutSeamFinder(cost_type=GRAD, stream=s).find(di, corners, dm)
    assert e.value.code == 3
    assert all(np.array_equal(_np(a), b) for a, b in zip(dm, masks))


def test_deterministic(gpu):
    corners, imgs, masks = layout(4, 3)
    dimgs = [_dev(a) for a in _f32(imgs)]
    want = model(4, 3)
    for _ in range(3):
        m = [_dev(x) for x in masks]
        gpu.GraphCutSeamFinder(cost_type=GRAD).find(dimgs, corners, m)
        assert all(np.array_equal(_np(a), b) for a, b in zip(m, want))


def test_cost_types_alternate_over_growing_and_shrinking_sets(gpu):
    """COST_COLOR (28 B per node) and COST_COLOR_GRAD (48 B) on one thread through the one grow-only scratch, 2, 4, then 2 host tiles,
    release() in between: every call equals its model."""
    pytest.importorskip("scipy")
    finders = {GG.COST_COLOR: gpu.GraphCutSeamFinder(), GRAD: gpu.GraphCutSeamFinder(cost_type=GRAD)}
    steps = [(2, 1, GG.COST_COLOR), (4, 3, GRAD), (2, 1, GRAD), (4, 3, GG.COST_COLOR), None, (3, 2, GRAD), (3, 2, GG.COST_COLOR), (2, 1, GRAD)]
    for step in steps:
        if step is None:
            gpu.GraphCutSeamFinder.release()
            continue
        n, seed, cost = step
        corners, imgs, masks = layout(n, seed)
        got = [m.copy() for m in masks]
        finders[cost].find(_f32(imgs), corners, got)
        for k, w in enumerate(model(n, seed, cost)):
            assert np.array_equal(got[k], w), (step, k, int((got[k] != w).sum()))


def test_two_threads_then_release(gpu):
    pytest.importorskip("scipy")
    cases = [(2, 1, GRAD), (3, 2, GG.COST_COLOR), (3, 2, GRAD)]
    want = [model(*c) for c in cases]
    done, errs = [0, 0], []

    def run(t):
        try:
            for it in range(4):
                k = (t + it) % len(cases)
                n, seed, cost = cases[k]
                corners, imgs, masks = layout(n, seed)
                m = [x.copy() for x in masks]
                gpu.GraphCutSeamFinder(cost_type=cost).find(_f32(imgs), corners, m)
                assert all(np.array_equal(a, b) for a, b in zip(m, want[k])), (t, it)
                done[t] += 1
            gpu.GraphCutSeamFinder.release()
        except Exception as e:                                       # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert done == [4, 4]


def test_cpp_graphcut_grad_demo(gpu, tmp_path):
    """tests/cpp/graphcut_grad_demo.cpp through isx::GraphCutSeamFinder(COST_COLOR_GRAD) and isx_cv::HipGraphCutSeamFinder(COST_COLOR_GRAD)
    (compiled against tests/cpp/opencv_stub with -Werror=suggest-override): both write the model's masks."""
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    exe = str(tmp_path / "graphcut_grad_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Wsuggest-override", "-Woverloaded-virtual", "-Werror=suggest-override",
                           "-Werror=overloaded-virtual", "-I", os.path.join(ROOT, "tests", "cpp", "opencv_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "graphcut_grad_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip",
                           "-Wl,-rpath," + lib_dir])
    corners, imgs, masks = layout(3, 2)
    want = model(3, 2)
    d = tmp_path / "in"
    d.mkdir()
    for k in range(3):
        imgs[k].tofile(str(d / ("img%d.bin" % k)))
        masks[k].tofile(str(d / ("mask%d.bin" % k)))
    args = [exe, str(d)] + ["%d %d %d %d" % (corners[k][0], corners[k][1], imgs[k].shape[1], imgs[k].shape[0]) for k in range(3)]
    out = subprocess.check_output(" ".join(args).split(), text=True, timeout=300)
    lines = [ln for ln in out.splitlines() if ln.startswith(("mirror", "adapter"))]
    assert len(lines) == 6, out
    for k in range(3):
        for kind in ("mirror", "adapter"):
            got = np.fromfile(str(d / ("%s%d.bin" % (kind, k))), np.uint8).reshape(masks[k].shape)
            assert np.array_equal(got, want[k]), (kind, k)


def test_end_to_end_feather_against_the_oracle(gpu, oracle):
    """W:223-313 on a reduced config-2 pair (960 x 540): warp (image + mask) -> convertTo(CV_32F) -> COST_COLOR_GRAD graph cut -> dilate
    20 x 20 & warped mask -> FeatherBlender(0.1), against the oracle's Feather on the model's seam masks.  The model's masks are the
    write-back of the labels that the pair's certificate proves on the model's graph: no pure-Python max-flow of a grid this size."""
    import torch
    W, H, F = 960, 540, 750.0
    K, Rs = synth.camera_pair(W, H, F)
    warper = gpu.CylindricalWarper().create(F)
    corners, warped, wmasks = [], [], []
    for i in range(2):
        c, wi, wm = warper.warp_with_mask(torch.from_numpy(synth.make_tile(H, W, 30 + i)).cuda(), K, Rs[i])
        corners.append(tuple(c)); warped.append(wi); wmasks.append(wm)
    f32 = [w.float() for w in warped]                                   # convertTo(CV_32F), W:261
    seam = [m.clone() for m in wmasks]                                  # masks_seam: W:247-249
    gpu.GraphCutSeamFinder(cost_type=GRAD).find(f32, corners, seam)     # W:258, W:264
    host_w, host_wm = [_np(w) for w in warped], [_np(m) for m in wmasks]
    want = [m.copy() for m in host_wm]
    r = check_pair(gpu, _np(f32[0]), _np(f32[1]), corners[0], corners[1], want[0], want[1])
    assert r is not None and r["rows"] * r["cols"] > 100_000
    assert all(np.array_equal(_np(a), b) for a, b in zip(seam, want))
    assert any((a != b).any() for a, b in zip(want, host_wm))
    sizes = [(w.shape[1], w.shape[0]) for w in host_w]
    fb = gpu.FeatherBlender(False, 0.1)
    fb.prepare(corners, sizes)
    ob = oracle.Feather(0.1)
    ob.prepare(corners, sizes)
    for i in range(2):
        dm = gpu.dilate_and(seam[i], 20, 20, wmasks[i])                 # W:286-301
        fb.feed_u8(warped[i], dm, corners[i])
        ob.feed(host_w[i].astype(np.int16), oracle.dilate_rect(want[i], 20, 20) & host_wm[i], corners[i])
    dst, dmask = fb.blend()
    odst, omask = ob.blend()
    assert np.array_equal(_np(dmask), omask)
    assert np.array_equal(_np(dst), odst)
