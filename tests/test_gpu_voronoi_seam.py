"""VoronoiSeamFinder on the GPU (isx_voronoi_seam_find) against the NumPy model of tests/helpers/voronoi_np.py, masks byte for byte: random
2-, 3- and 4-tile layouts (host, device, pitched and unaligned mats), the reference's tiles, a full 4K pair, degenerate rois, the float /
integer trap past 8192 cells, a captured warp -> find -> dilate & AND -> multi-band cycle replayed on rewritten masks, determinism, threads,
the error paths, the C++ mirror and OpenCV adapter, and warp -> gain -> Voronoi -> dilate & AND -> Feather against the oracle."""
import gc
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import guarded  # noqa: E402
from helpers import voronoi_np as V  # noqa: E402
from imagestitch_amd import synth  # noqa: E402
from test_voronoi_model import REF_NONZERO_AFTER, REF_ROI, REF_SEAM_CELLS  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_SIZE = 1, 2, 3, 7


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _sizes(masks):
    return [(int(m.shape[1]), int(m.shape[0])) for m in masks]


def layout(n, seed):
    """n tiles of assorted sizes that overlap in many ways, masks with holes (the pattern of tests/test_gpu_graphcut_seam.py)."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(40, 90)), int(rng.integers(30, 70))) for _ in range(n)]
    corners = [(int(rng.integers(-30, 30)), int(rng.integers(-20, 20))) for _ in range(n)]
    masks = []
    for w, h in sizes:
        m = np.full((h, w), 255, np.uint8)
        for _ in range(3):
            y, x = int(rng.integers(0, h - 4)), int(rng.integers(0, w - 4))
            m[y:y + int(rng.integers(2, 10)), x:x + int(rng.integers(2, 10))] = 0
        m[m != 0] = rng.integers(1, 256, int((m != 0).sum()))           # any non-zero byte is "set"
        masks.append(m)
    return corners, masks


def model(corners, masks):
    out = [np.array(_np(m)).copy() for m in masks]
    V.find(_sizes(out), corners, out)
    return out


def views(arrays, where, seed):
    """Each array inside a guard band of seeded random bytes (tests/helpers/guarded.py, the "odd" layout: an unaligned first byte, a
    pitch that is no multiple of 16)."""
    return [guarded.guarded_like(a, where, "odd", 100 * seed + k) for k, a in enumerate(arrays)]


def check(gpu, corners, masks, where="device"):
    want = model(corners, masks)
    got = [_dev(m) for m in masks] if where == "device" else [m.copy() for m in masks]
    gpu.VoronoiSeamFinder().find(_sizes(masks), corners, got)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(_np(g), w), (k, int((_np(g) != w).sum()))
    return want


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3)])
@pytest.mark.parametrize("where", ["host", "device", "host_view", "device_view"])
def test_model_parity(gpu, n, seed, where):
    corners, masks = layout(n, seed)
    want = model(corners, masks)
    assert any((w != m).any() for w, m in zip(want, masks))          # the seams cut something
    if where in ("host", "device"):
        check(gpu, corners, masks, where)
        return
    vs = views(masks, where.split("_")[0], seed)
    gpu.VoronoiSeamFinder().find(_sizes(masks), corners, [g.view for g in vs])
    for k, g in enumerate(vs):
        assert np.array_equal(_np(g.view), want[k]), (k, int((_np(g.view) != want[k]).sum()))
        g.check()                                                     # nothing around the view was written


def test_src_form_takes_sizes_from_the_images(gpu):
    corners, masks = layout(3, 2)
    want = model(corners, masks)
    src = [np.zeros(m.shape + (3,), np.float32) for m in masks]
    got = [_dev(m) for m in masks]
    assert gpu.VoronoiSeamFinder().find(src, corners, got) is got
    assert all(np.array_equal(_np(g), w) for g, w in zip(got, want))


def test_reference_tiles(gpu):
    """The reference's tiles' masks as they went into its seam finder: the counts pinned in tests/test_voronoi_model.py."""
    from test_ref_artifact import dpseam_case
    c = dpseam_case()
    masks = [np.array(m) for m in c["masks_in"]]
    assert V.overlap_roi(c["corners"][0], c["corners"][1], *_sizes(masks)) == REF_ROI
    for where in ("host", "device"):
        want = check(gpu, c["corners"], masks, where)
        assert tuple(int((m != 0).sum()) for m in want) == REF_NONZERO_AFTER
    x0, y0, w, h = REF_ROI
    tl = c["corners"][1]
    cleared = (masks[1] != 0) & (want[1] == 0)
    assert not cleared[:, :x0 - tl[0]].any() and int(cleared.sum()) <= REF_SEAM_CELLS


def _warped_4k_pair(gpu):
    import torch
    W, H, F = 3840, 2160, 3000.0
    K, Rs = synth.camera_pair(W, H, F)
    warper = gpu.CylindricalWarper().create(F)
    corners, wms = [], []
    for i in range(2):
        c, _, wm = warper.warp_with_mask(torch.from_numpy(synth.make_tile(H, W, 20 + i)).cuda(), K, Rs[i])
        corners.append(tuple(c)); wms.append(wm)
    torch.cuda.synchronize()
    return corners, wms


def test_full_4k_pair(gpu):
    """One 4K pair (3840 x 2160, f = 3000) warped on the GPU, device-resident."""
    corners, wms = _warped_4k_pair(gpu)
    host = [_np(m) for m in wms]
    roi = V.overlap_roi(corners[0], corners[1], *_sizes(host))
    assert roi[2] * roi[3] > 2_000_000
    want = model(corners, host)
    gpu.VoronoiSeamFinder().find(_sizes(host), corners, wms)
    assert np.array_equal(_np(wms[0]), want[0]) and np.array_equal(_np(wms[1]), want[1])
    assert (want[0] != host[0]).any() and (want[1] != host[1]).any()


def _holes(shape, seed, p=0.1):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < p, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("name,sizes,corners", [
    ("1x1 overlap", [(9, 7), (8, 6)], [(0, 0), (8, 6)]),
    ("1 cell wide", [(20, 40), (30, 25)], [(0, 0), (19, 5)]),
    ("1 cell high", [(40, 20), (25, 30)], [(0, 0), (5, 19)]),
    ("narrower than a wave", [(50, 300), (45, 280)], [(0, 0), (40, 11)]),
    ("wider than one row-pass chunk", [(5000, 12), (4700, 9)], [(0, 0), (150, 5)]),
    ("wider than two chunks", [(9000, 5), (9100, 6)], [(0, 0), (-30, -2)]),
    ("taller than many segments", [(12, 3000), (9, 2800)], [(0, 0), (5, 100)]),
    ("disjoint", [(30, 20), (30, 20)], [(0, 0), (30, 0)]),
    ("identical tiles", [(33, 21), (33, 21)], [(4, -2), (4, -2)]),
    ("one inside the other", [(120, 90), (31, 17)], [(0, 0), (40, 30)]),
])
def test_degenerate_rois(gpu, name, sizes, corners):
    for holes in (False, True):
        masks = [_holes((h, w), 5 + k) if holes else np.full((h, w), 255, np.uint8) for k, (w, h) in enumerate(sizes)]
        want = check(gpu, corners, masks)
        if name == "disjoint":
            assert all(np.array_equal(w, m) for w, m in zip(want, masks))
        check(gpu, corners, masks, "host")


def test_rows_with_no_unique_cell(gpu):
    """Rows of the overlap in which neither tile has a cell of its own, and a mask that is empty."""
    sizes, corners = [(60, 40), (60, 40)], [(0, 0), (0, 12)]
    m0, m1 = np.full((40, 60), 255, np.uint8), np.full((40, 60), 255, np.uint8)
    m0[:, :30] = 0
    m1[:, :30] = 0
    check(gpu, corners, [m0, m1])
    check(gpu, corners, [np.zeros((40, 60), np.uint8), m1])
    check(gpu, corners, [m0, np.zeros((40, 60), np.uint8)])
    check(gpu, corners, [np.zeros((40, 60), np.uint8), np.zeros((40, 60), np.uint8)])
    del sizes


def test_fewer_than_two_images(gpu):
    f = gpu.VoronoiSeamFinder()
    assert f.find([], [], []) == []
    m = [_dev(np.full((5, 7), 255, np.uint8))]
    f.find([(7, 5)], [(0, 0)], m)
    assert (_np(m[0]) == 255).all()


def test_float_comparison_past_8192_cells(gpu):
    """tests/test_voronoi_model.py's strip: a submask 9020 cells wide, tile 1 without a cell of its own.  Where tile 2's distance is
    8192 + the ring distance the two 16.16 integers differ by one and the floats are equal: comparing integers would clear tile 2 there."""
    sizes, corners = [(9000, 3), (9001, 3)], [(0, 0), (0, 0)]
    masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
    want = check(gpu, corners, masks)
    assert not want[0].any() and (want[1] == 255).all()
    # and with tile 1 owning cells far to the left, so that both branches occur along the strip
    sizes, corners = [(9000, 3), (8990, 3)], [(0, 0), (10, 0)]
    masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
    masks[0][:, 5:10] = 0
    want = check(gpu, corners, masks)
    assert want[0].any() and want[1].any()


def test_deterministic(gpu):
    corners, masks = layout(4, 3)
    want = model(corners, masks)
    f = gpu.VoronoiSeamFinder()
    for _ in range(50):
        m = [_dev(x) for x in masks]
        f.find(_sizes(masks), corners, m)
        assert all(np.array_equal(_np(a), b) for a, b in zip(m, want))


def test_two_threads_then_release(gpu):
    import torch
    cases = [layout(2, 1), layout(3, 2)]
    want = [model(*c) for c in cases]
    done, errs = [False, False], []

    def run(k):
        try:
            corners, masks = cases[k]
            s = torch.cuda.Stream()
            f = gpu.VoronoiSeamFinder(stream=s)
            for _ in range(20):
                with torch.cuda.stream(s):
                    m = [_dev(x) for x in masks]
                    f.find(_sizes(masks), corners, m)
                s.synchronize()
                assert all(np.array_equal(_np(a), b) for a, b in zip(m, want[k]))
            gpu.VoronoiSeamFinder.release()
            done[k] = True
        except Exception as e:                                       # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert all(done)


def test_release_then_find(gpu):
    corners, masks = layout(3, 2)
    check(gpu, corners, masks)
    gpu.VoronoiSeamFinder.release()
    gpu.VoronoiSeamFinder.release()
    check(gpu, corners, masks)
    check(gpu, corners, masks, "host")


def test_errors_leave_the_masks_untouched(gpu):
    import ctypes as C
    import torch
    from imagestitch_amd import _lib
    corners, masks = layout(3, 2)
    sizes = _sizes(masks)
    f = gpu.VoronoiSeamFinder()

    def refused(code, sz, cs, ms):
        with pytest.raises(gpu.IsxError) as e:
            f.find(sz, cs, ms)
        assert e.value.code == code, e.value
        assert all(np.array_equal(_np(a), b) for a, b in zip(m, masks))

    for where in ("host", "device"):
        m = [x.copy() for x in masks] if where == "host" else [_dev(x) for x in masks]
        bad = list(sizes)
        bad[2] = (sizes[2][0] + 1, sizes[2][1])                     # the LAST mask differs from its size: refused before pair (0, 1) writes
        refused(ERR_SIZE, bad, corners, m)
        bad[2] = (sizes[2][0], sizes[2][1] - 1)
        refused(ERR_SIZE, bad, corners, m)
        bad[2] = (-1, sizes[2][1])
        refused(ERR_INVALID, bad, corners, m)
        wrong = m[:2] + [np.zeros(masks[2].shape + (3,), np.uint8) if where == "host" else _dev(np.zeros(masks[2].shape + (3,), np.uint8))]
        refused(ERR_TYPE, sizes, corners, wrong)
        refused(ERR_INVALID, sizes, corners[:2], m)                  # lengths differ: refused by the wrapper
    lib = _lib.load()
    mats = (_lib.IsxMat * 3)(*[_lib.as_mat(x) for x in masks])
    ints = (C.c_int * 6)(*[v for s in sizes for v in s])
    assert lib.isx_voronoi_seam_find(3, None, ints, mats, 0, None) == ERR_INVALID
    assert lib.isx_voronoi_seam_find(3, ints, None, mats, 0, None) == ERR_INVALID
    assert lib.isx_voronoi_seam_find(3, ints, ints, None, 0, None) == ERR_INVALID
    assert lib.isx_voronoi_seam_find(-1, ints, ints, mats, 0, None) == ERR_INVALID
    assert lib.isx_voronoi_seam_reserve(0, 5, 0) == ERR_INVALID and lib.isx_voronoi_seam_reserve(5, -1, 0) == ERR_INVALID
    torch.cuda.synchronize()


def _capture_rig(gpu):
    """Two 640 x 360 tiles, their planned ROIs, resident outputs, a warper and a 4-band F32 blender on one side stream."""
    import torch
    W, H, F = 640, 360, 500.0
    K, Rs = synth.camera_pair(W, H, F)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    r = dict(W=W, H=H, F=F, K=K, Rs=Rs, s=s)
    r["host_imgs"] = [synth.make_tile(H, W, 40 + i) for i in range(2)]
    warper = gpu.CylindricalWarper(0, s).create(F)
    warper.set_deferred_verify(True)
    r["rois"] = [warper.warpRoi((W, H), K, R) for R in Rs]
    r["sizes"] = [(q[2] - q[0] + 1, q[3] - q[1] + 1) for q in r["rois"]]
    r["corners"] = [(q[0], q[1]) for q in r["rois"]]
    with torch.cuda.stream(s):
        r["imgs"] = [torch.from_numpy(a).cuda() for a in r["host_imgs"]]
        r["src_masks"] = [torch.full((H, W), 255, dtype=torch.uint8, device="cuda") for _ in range(2)]
        r["warped"] = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for w, h in r["sizes"]]
        r["wmasks"] = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for w, h in r["sizes"]]
        r["seam"] = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for w, h in r["sizes"]]
    blender = gpu.MultiBandBlender(False, 4, gpu.PREC_F32, 0, s)
    blender.set_deferred_level0(True)
    blender.prepare(r["corners"], r["sizes"])
    fw, fh = blender.result_size()
    with torch.cuda.stream(s):
        r["out"] = torch.zeros((fh, fw, 3), dtype=torch.float32, device="cuda")
        r["out_mask"] = torch.zeros((fh, fw), dtype=torch.uint8, device="cuda")
    r["warper"], r["blender"] = warper, blender
    r["finder"] = gpu.VoronoiSeamFinder(stream=s)
    return r


def _chain(gpu, r):
    """warp (image + the caller's mask) -> masks_seam = the warped masks -> Voronoi -> dilate 20 x 20 & warped mask -> feed -> blend,
    all on r["s"]; the dilated masks are kept alive until blend() has read them (deferred level 0)."""
    for i in range(2):
        r["warper"].warp_with_mask_planned(r["imgs"][i], r["K"], r["Rs"][i], r["rois"][i], r["warped"][i], r["wmasks"][i], mask=r["src_masks"][i])
    r["warper"].discard_pending()          # the plan's verification is not part of this chain
    for i in range(2):
        r["seam"][i].copy_(r["wmasks"][i])
    r["finder"].find(r["sizes"], r["corners"], r["seam"])
    r["blender"].prepare(r["corners"], r["sizes"])
    r["dil"] = [gpu.dilate_and(r["seam"][i], 20, 20, r["wmasks"][i], stream=r["s"]) for i in range(2)]
    for i in range(2):
        r["blender"].feed_u8(r["warped"][i], r["dil"][i], r["corners"][i])
    r["blender"].blend(r["out"], r["out_mask"])


def _chain_model(oracle, r, src_masks):
    ob = oracle.MultiBand(4, 1)
    ob.prepare(r["corners"], r["sizes"])
    wis, wms = [], []
    for i in range(2):
        oc, owi, _ = oracle.warp_u8(0, r["F"], r["K"], r["Rs"][i], r["host_imgs"][i], 1, 2)
        _, owm, _ = oracle.warp_u8(0, r["F"], r["K"], r["Rs"][i], src_masks[i], 0, 0)
        assert oc == tuple(r["corners"][i])
        wis.append(owi); wms.append(owm)
    seam = model(r["corners"], wms)
    for i in range(2):
        ob.feed(wis[i].astype(np.int16), oracle.dilate_rect(seam[i], 20, 20) & wms[i], r["corners"][i])
    return seam, ob.blend(True)


def _src_masks(H, W, k):
    m = [np.full((H, W), 255, np.uint8) for _ in range(2)]
    if k:
        rng = np.random.default_rng(100 + k)
        for a in m:
            for _ in range(6):
                y, x = int(rng.integers(0, H - 60)), int(rng.integers(0, W - 80))
                a[y:y + int(rng.integers(10, 60)), x:x + int(rng.integers(10, 80))] = 0
    return m


def test_captured_chain_replays_on_rewritten_masks(gpu, oracle):
    """reserve, then warp -> find -> dilate & AND -> feed -> blend captured on a side stream as one chain; three replays, the tiles' source
    masks rewritten before each: every replay equals the eager chain on the same masks and the model."""
    import torch
    r = _capture_rig(gpu)
    s = r["s"]
    roi = V.overlap_roi(r["corners"][0], r["corners"][1], *r["sizes"])
    gpu.VoronoiSeamFinder.release()
    r["finder"].reserve(roi[2], roi[3])
    with torch.cuda.stream(s):
        _chain(gpu, r)                                                # warm-up: tables, buffers
    r["warper"].join()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    # a CUDAGraph that a dead reference cycle still holds (a test frame kept by its own pytest.raises info) must not be freed by a collection
    # that happens to run inside this capture: its destructor synchronises the device, which a capturing stream turns into an abort
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        _chain(gpu, r)
    for k in range(3):
        src = _src_masks(r["H"], r["W"], k + 1)
        with torch.cuda.stream(s):
            for i in range(2):
                r["src_masks"][i].copy_(torch.from_numpy(src[i]).cuda())
            for t in r["seam"] + [r["out"], r["out_mask"]]:
                t.zero_()
        s.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got_seam = [_np(t).copy() for t in r["seam"]]
        got_out, got_mask = _np(r["out"]).copy(), _np(r["out_mask"]).copy()
        want_seam, (od, om) = _chain_model(oracle, r, src)
        assert all(np.array_equal(a, b) for a, b in zip(got_seam, want_seam)), k
        assert np.array_equal(got_mask, om) and np.array_equal(got_out, od), k
        assert any((a != _np(w)).any() for a, w in zip(got_seam, r["wmasks"]))       # the finder cut something
        with torch.cuda.stream(s):                                     # the eager chain on the same inputs
            for t in r["seam"] + [r["out"], r["out_mask"]]:
                t.zero_()
            _chain(gpu, r)
        r["warper"].join()
        torch.cuda.synchronize()
        assert all(np.array_equal(_np(t), b) for t, b in zip(r["seam"], got_seam)), k
        assert np.array_equal(_np(r["out"]), got_out) and np.array_equal(_np(r["out_mask"]), got_mask), k


def test_captured_find_refuses_host_masks_and_missing_scratch(gpu):
    """On a capturing stream: host masks, and device masks that need more scratch than was reserved, give ISX_ERR_STATE with nothing
    enqueued; the capture stays usable and a find that fits is captured after them."""
    import torch
    corners, masks = layout(2, 1)
    sizes = _sizes(masks)
    want = model(corners, masks)
    big_c, big_m = [(0, 0), (10, 10)], [np.full((1200, 1500), 255, np.uint8) for _ in range(2)]
    roi = V.overlap_roi(corners[0], corners[1], *sizes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    f = gpu.VoronoiSeamFinder(stream=s)
    gpu.VoronoiSeamFinder.release()
    with torch.cuda.stream(s):
        dm, dbig = [_dev(m) for m in masks], [_dev(m) for m in big_m]
        x = torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(gpu.IsxError) as e:                        # nothing reserved at all
            f.find(sizes, corners, dm)
        assert e.value.code == ERR_STATE and "captur" in e.value.msg, e.value.msg
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0 and all(np.array_equal(_np(a), b) for a, b in zip(dm, masks))
    f.reserve(roi[2], roi[3])
    host = [m.copy() for m in masks]
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(gpu.IsxError) as e:
            f.find(sizes, corners, host)
        assert e.value.code == ERR_STATE and "host" in e.value.msg, e.value.msg
        with pytest.raises(gpu.IsxError) as e:
            f.find(_sizes(big_m), big_c, dbig)
        assert e.value.code == ERR_STATE and "reserve" in e.value.msg, e.value.msg
        f.find(sizes, corners, dm)
    assert all(np.array_equal(a, b) for a, b in zip(host, masks))
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 2.0
    assert all(np.array_equal(_np(a), b) for a, b in zip(dm, want))
    assert all(np.array_equal(_np(a), b) for a, b in zip(dbig, big_m))
    del g
    gpu.VoronoiSeamFinder.release()


def test_cpp_voronoi_demo(gpu, tmp_path):
    """tests/cpp/voronoi_demo.cpp through isx::VoronoiSeamFinder (both find forms) and isx_cv::HipVoronoiSeamFinder
    (include/imagestitch_cv_seam.hpp, compiled against tests/cpp/opencv_stub with -Werror=suggest-override): the masks equal the model's."""
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    exe = str(tmp_path / "voronoi_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Wsuggest-override", "-Woverloaded-virtual", "-Werror=suggest-override",
                           "-Werror=overloaded-virtual", "-I", os.path.join(ROOT, "tests", "cpp", "opencv_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "voronoi_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip",
                           "-Wl,-rpath," + lib_dir])
    corners, masks = layout(3, 2)
    want = model(corners, masks)
    d = tmp_path / "in"
    d.mkdir()
    for k in range(3):
        masks[k].tofile(str(d / ("mask%d.bin" % k)))
    args = [exe, str(d)] + ["%d %d %d %d" % (corners[k][0], corners[k][1], masks[k].shape[1], masks[k].shape[0]) for k in range(3)]
    out = subprocess.check_output(" ".join(args).split(), text=True, timeout=300)
    lines = [ln for ln in out.splitlines() if ln.startswith(("mirror", "sizes", "adapter"))]
    assert len(lines) == 9, out
    for ln in lines:
        kind, k, total = ln.split()
        assert int(total) == int(want[int(k)].astype(np.int64).sum()), ln
    for k in range(3):
        for kind in ("mirror", "sizes", "adapter"):
            got = np.fromfile(str(d / ("%s%d.bin" % (kind, k))), np.uint8).reshape(masks[k].shape)
            assert np.array_equal(got, want[k]), (kind, k)


def test_end_to_end_feather_against_the_oracle(gpu, oracle):
    """S:1156-1283 on a reduced pair: warp (image + mask) -> gain feed + apply -> Voronoi -> dilate 20 x 20 & warped mask ->
    FeatherBlender(0.1), against the oracle's Feather on the model's seam masks."""
    import torch
    W, H, F = 960, 540, 750.0
    K, Rs = synth.camera_pair(W, H, F)
    warper = gpu.CylindricalWarper().create(F)
    corners, warped, wmasks = [], [], []
    for i in range(2):
        c, wi, wm = warper.warp_with_mask(torch.from_numpy(synth.make_tile(H, W, 30 + i)).cuda(), K, Rs[i])
        corners.append(tuple(c)); warped.append(wi); wmasks.append(wm)
    comp = gpu.GainCompensator().feed(corners, warped, wmasks)
    for i in range(2):
        comp.apply(i, corners[i], warped[i], wmasks[i])
    seam = [m.clone() for m in wmasks]                                  # masks_seam
    gpu.VoronoiSeamFinder().find(warped, corners, seam)                 # S:1180, S:1192
    host_w, host_wm = [_np(w) for w in warped], [_np(m) for m in wmasks]
    want = model(corners, host_wm)
    assert all(np.array_equal(_np(a), b) for a, b in zip(seam, want))
    sizes = _sizes(host_wm)
    fb = gpu.FeatherBlender(False, 0.1)
    fb.prepare(corners, sizes)
    ob = oracle.Feather(0.1)
    ob.prepare(corners, sizes)
    for i in range(2):
        dm = gpu.dilate_and(seam[i], 20, 20, wmasks[i])
        fb.feed_u8(warped[i], dm, corners[i])
        ob.feed(host_w[i].astype(np.int16), oracle.dilate_rect(want[i], 20, 20) & host_wm[i], corners[i])
    dst, dmask = fb.blend()
    odst, omask = ob.blend()
    assert np.array_equal(_np(dmask), omask)
    assert np.array_equal(_np(dst), odst)


def test_mixed_residency(gpu):
    """Masks 0 and 2 on the host, mask 1 on the device: the host masks are copied back, the device mask is edited in place."""
    corners, masks = layout(3, 2)
    want = model(corners, masks)
    assert all((w != m).any() for w, m in zip(want, masks))           # every tile's mask is cut: each copy-back shows
    mk = [_dev(m) if k == 1 else m.copy() for k, m in enumerate(masks)]
    assert gpu.VoronoiSeamFinder().find(_sizes(masks), corners, mk) is mk
    assert isinstance(mk[0], np.ndarray) and mk[1].is_cuda and isinstance(mk[2], np.ndarray)
    for k in range(3):
        assert np.array_equal(_np(mk[k]), want[k]), (k, int((_np(mk[k]) != want[k]).sum()))


def test_growing_and_shrinking_sets_on_one_thread(gpu):
    """2, 5, then 2 host masks through one finder on one thread (the staged copies of a tile index change size and count), then release()
    and one more call: every call equals the model."""
    f = gpu.VoronoiSeamFinder()
    for n, seed in [(2, 1), (5, 4), (2, 1), (0, 0), (3, 2)]:
        if n == 0:
            f.release()
            continue
        corners, masks = layout(n, seed)
        want = model(corners, masks)
        got = [m.copy() for m in masks]
        f.find(_sizes(masks), corners, got)
        for k in range(n):
            assert np.array_equal(got[k], want[k]), (n, k, int((got[k] != want[k]).sum()))
