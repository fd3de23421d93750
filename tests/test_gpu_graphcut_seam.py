"""GraphCutSeamFinder(COST_COLOR) on the GPU (isx_graphcut_seam_find) against the NumPy model of tests/helpers/graphcut_np.py: masks byte
for byte on random 2-, 3- and 4-tile layouts (F32 and U8 tiles; host, device, pitched and unaligned mats), a certificate of every pair's
maximum flow and maximal cut checked in NumPy (the full 4K pair included), the reference's tiles, determinism, the error paths, threads,
the C++ mirror and OpenCV adapter, and warp -> gain -> graph cut -> dilate & AND -> Feather against the oracle."""
import gc
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import graphcut_np as G  # noqa: E402
from helpers import guarded  # noqa: E402
from imagestitch_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def layout(n, seed):
    """n tiles of assorted sizes that overlap in many ways, smooth-ish colours (so that seams have room to move), masks with holes."""
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


def model(corners, imgs, masks):
    pytest.importorskip("scipy")
    out = [m.copy() for m in masks]
    G.find([_np(a) for a in imgs], corners, out)
    return out


def views(arrays, where, seed):
    """Each array inside a guard band of seeded random bytes (tests/helpers/guarded.py, the "odd" layout: an unaligned first byte for U8,
    a pitch that is no multiple of 16)."""
    return [guarded.guarded_like(a, where, "odd", 100 * seed + k) for k, a in enumerate(arrays)]


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3)])
@pytest.mark.parametrize("depth", ["u8", "f32"])
@pytest.mark.parametrize("where", ["host", "device", "host_view", "device_view"])
def test_model_parity(gpu, n, seed, depth, where):
    corners, imgs, masks = layout(n, seed)
    want = model(corners, imgs, masks)
    assert any((w != m).any() for w, m in zip(want, masks))          # the seams cut something
    src = [a.astype(np.float32) for a in imgs] if depth == "f32" else imgs
    if where in ("host", "device"):
        src_v = [_dev(a) for a in src] if where == "device" else [a.copy() for a in src]
        mk_v = [_dev(m) for m in masks] if where == "device" else [m.copy() for m in masks]
    else:
        kind = where.split("_")[0]
        g_src, g_mk = views(src, kind, seed), views(masks, kind, seed + 1)
        src_v, mk_v = [g.view for g in g_src], [g.view for g in g_mk]
    gpu.GraphCutSeamFinder().find(src_v, corners, mk_v)
    for k in range(n):
        assert np.array_equal(_np(mk_v[k]), want[k]), (k, int((_np(mk_v[k]) != want[k]).sum()))
    if where not in ("host", "device"):
        for g in g_mk:
            g.check()                                                # nothing around a mask was written
        for g in g_src:
            g.check(guarded.NOTHING)                                 # ... and the images are inputs


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3), (2, 9)])
def test_certificate_of_every_pair(gpu, n, seed):
    """The one-pair form on every overlapping pair in find()'s order: its certificate proves a maximum flow and the maximal minimum
    cut of the model's graph (NumPy only), and its masks continue the sequence find() produces."""
    corners, imgs, masks = layout(n, seed)
    ms = [m.copy() for m in masks]
    sizes = [(a.shape[1], a.shape[0]) for a in imgs]
    fdr = gpu.GraphCutSeamFinder()
    pairs = 0
    for i in range(n - 1):
        for j in range(i + 1, n):
            roi = G.overlap_roi(corners[i], corners[j], sizes[i], sizes[j])
            g = G.pair_graph(imgs[i], imgs[j], ms[i], ms[j], corners[i], corners[j], roi) if roi else None
            r = fdr.find_pair(imgs[i], imgs[j], corners[i], corners[j], ms[i], ms[j], certificate=True)
            if roi is None:
                assert r["rows"] == 0 and r["flow"] == 0
                continue
            pairs += 1
            assert (r["rows"], r["cols"]) == (roi[3] + 20, roi[2] + 20)
            G.check_certificate(g, r["flow"], r["residuals"], r["labels"])
            assert r["rounds"] >= 0 and r["launches"] > 0
    assert pairs >= 1
    got = [m.copy() for m in masks]
    fdr.find(imgs, corners, got)
    assert all(np.array_equal(a, b) for a, b in zip(got, ms))


def test_reference_tiles(gpu):
    """The reference's warped tiles (CV_32FC3) with the masks that went into its seam finder: maximum flow 211 105, masks equal the
    model's; the same as device mats."""
    from test_ref_artifact import dpseam_case
    c = dpseam_case()
    want = model(c["corners"], c["images"], c["masks_in"])
    fdr = gpu.GraphCutSeamFinder()
    m = [x.copy() for x in c["masks_in"]]
    r = fdr.find_pair(c["images"][0], c["images"][1], c["corners"][0], c["corners"][1], m[0], m[1], certificate=True)
    assert r["flow"] == 211105 and (r["rows"], r["cols"]) == (1117, 307)
    assert int(r["labels"].sum()) == 152666
    assert np.array_equal(m[0], want[0]) and np.array_equal(m[1], want[1])
    md = [_dev(x) for x in c["masks_in"]]
    fdr.find([_dev(a) for a in c["images"]], c["corners"], md)
    assert np.array_equal(_np(md[0]), want[0]) and np.array_equal(_np(md[1]), want[1])


def _warped_4k_pair(gpu):
    import torch
    W, H, F = 3840, 2160, 3000.0
    K, Rs = synth.camera_pair(W, H, F)
    warper = gpu.CylindricalWarper().create(F)
    corners, wis, wms = [], [], []
    for i in range(2):
        c, wi, wm = warper.warp_with_mask(torch.from_numpy(synth.make_tile(H, W, 20 + i)).cuda(), K, Rs[i])
        corners.append(tuple(c)); wis.append(wi); wms.append(wm)
    torch.cuda.synchronize()
    return corners, wis, wms


def test_full_4k_pair_certificate(gpu):
    """One 4K pair (3840 x 2160, f = 3000) warped on the GPU, device-resident: the certificate against the model's graph."""
    corners, wis, wms = _warped_4k_pair(gpu)
    host_i, host_m = [_np(a) for a in wis], [_np(m) for m in wms]
    sizes = [(a.shape[1], a.shape[0]) for a in host_i]
    roi = G.overlap_roi(corners[0], corners[1], sizes[0], sizes[1])
    g = G.pair_graph(host_i[0], host_i[1], host_m[0], host_m[1], corners[0], corners[1], roi)
    r = gpu.GraphCutSeamFinder().find_pair(wis[0], wis[1], corners[0], corners[1], wms[0], wms[1], certificate=True)
    assert r["rows"] * r["cols"] > 2_000_000
    G.check_certificate(g, r["flow"], r["residuals"], r["labels"])
    m0, m1 = host_m[0].copy(), host_m[1].copy()
    G.write_back(r["labels"], m0, m1, corners[0], corners[1], roi)
    assert np.array_equal(_np(wms[0]), m0) and np.array_equal(_np(wms[1]), m1)


def test_deterministic(gpu):
    corners, imgs, masks = layout(4, 3)
    dimgs = [_dev(a) for a in imgs]
    first = None
    for _ in range(4):
        m = [_dev(x) for x in masks]
        gpu.GraphCutSeamFinder().find(dimgs, corners, m)
        got = [_np(x) for x in m]
        if first is None:
            first = got
        assert all(np.array_equal(a, b) for a, b in zip(first, got))


def test_errors_leave_the_masks_untouched(gpu):
    import torch
    corners, imgs, masks = layout(3, 2)
    f32 = [a.astype(np.float32) for a in imgs]
    f32[2][5, 7, 1] += 0.5                                          # read by the last pair only: still refused before the first writes
    for where in ("host", "device"):
        m = [x.copy() for x in masks] if where == "host" else [_dev(x) for x in masks]
        src = f32 if where == "host" else [_dev(a) for a in f32]
        with pytest.raises(gpu.IsxError) as e:
            gpu.GraphCutSeamFinder().find(src, corners, m)
        assert e.value.code == 6
        assert all(np.array_equal(_np(a), b) for a, b in zip(m, masks))
    m = [x.copy() for x in masks]
    with pytest.raises(gpu.IsxError) as e:
        gpu.GraphCutSeamFinder(cost_type=gpu.seam.COST_COLOR_GRAD).find(imgs, corners, m)
    assert e.value.code == 6 and all(np.array_equal(a, b) for a, b in zip(m, masks))
    # a capturing stream: ISX_ERR_STATE before anything is enqueued
    dm, di = [_dev(x) for x in masks], [_dev(a) for a in imgs]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    # a CUDAGraph that a dead reference cycle still holds (a test frame kept by its own pytest.raises info) must not be freed by a collection
    # that happens to run inside this capture: its destructor synchronises the device, which a capturing stream turns into an abort
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        with pytest.raises(gpu.IsxError) as e:
            gpu.GraphCutSeamFinder(stream=s).find(di, corners, dm)
    assert e.value.code == 3
    assert all(np.array_equal(_np(a), b) for a, b in zip(dm, masks))


def test_two_threads_then_release(gpu):
    cases = [layout(2, 1), layout(3, 2)]
    want = [model(*c) for c in cases]
    got, errs = [None, None], []

    def run(k):
        try:
            corners, imgs, masks = cases[k]
            for _ in range(3):
                m = [x.copy() for x in masks]
                gpu.GraphCutSeamFinder().find(imgs, corners, m)
                assert all(np.array_equal(a, b) for a, b in zip(m, want[k]))
            got[k] = m
            gpu.GraphCutSeamFinder.release()
        except Exception as e:                                       # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert got[0] is not None and got[1] is not None


def test_cpp_graphcut_demo(gpu, tmp_path):
    """tests/cpp/graphcut_demo.cpp through isx::GraphCutSeamFinder and isx_cv::HipGraphCutSeamFinder (include/imagestitch_cv_seam.hpp,
    compiled against tests/cpp/opencv_stub with -Werror=suggest-override): both print the masks' digests, which equal the model's."""
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    exe = str(tmp_path / "graphcut_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Wsuggest-override", "-Woverloaded-virtual", "-Werror=suggest-override",
                           "-Werror=overloaded-virtual", "-I", os.path.join(ROOT, "tests", "cpp", "opencv_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "graphcut_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip",
                           "-Wl,-rpath," + lib_dir])
    corners, imgs, masks = layout(3, 2)
    want = model(corners, [a.astype(np.float32) for a in imgs], masks)
    d = tmp_path / "in"
    d.mkdir()
    for k in range(3):
        imgs[k].tofile(str(d / ("img%d.bin" % k)))
        masks[k].tofile(str(d / ("mask%d.bin" % k)))
    args = [exe, str(d)] + ["%d %d %d %d" % (corners[k][0], corners[k][1], imgs[k].shape[1], imgs[k].shape[0]) for k in range(3)]
    out = subprocess.check_output(" ".join(args).split(), text=True, timeout=300)
    lines = [ln for ln in out.splitlines() if ln.startswith(("mirror", "adapter"))]
    assert len(lines) == 6, out
    for ln in lines:
        kind, k, total = ln.split()
        assert int(total) == int(want[int(k)].astype(np.int64).sum()), (ln, int(want[int(k)].astype(np.int64).sum()))
    for k in range(3):
        for kind in ("mirror", "adapter"):
            got = np.fromfile(str(d / ("%s%d.bin" % (kind, k))), np.uint8).reshape(masks[k].shape)
            assert np.array_equal(got, want[k]), (kind, k)


def test_end_to_end_feather_against_the_oracle(gpu, oracle):
    """W:223-313 on a reduced config-2 pair: warp (image + mask) -> gain feed + apply -> convertTo(CV_32F) -> graph cut -> dilate 20 x 20
    & warped mask -> FeatherBlender(0.1), against the oracle's Feather on the model's seam masks."""
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
    seam = [m.clone() for m in wmasks]                                  # masks_seam: W:247-249
    f32 = [w.float() for w in warped]                                   # convertTo(CV_32F), W:261
    gpu.GraphCutSeamFinder().find(f32, corners, seam)                   # W:257, W:264
    host_w, host_wm = [_np(w) for w in warped], [_np(m) for m in wmasks]
    want = model(corners, [a.astype(np.float32) for a in host_w], host_wm)
    assert all(np.array_equal(_np(a), b) for a, b in zip(seam, want))
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


def test_mixed_residency(gpu):
    """Tiles 0 and 2 on the host, tile 1 on the device: the host masks are copied back, the device mask is edited in place."""
    corners, imgs, masks = layout(3, 2)
    want = model(corners, imgs, masks)
    assert all((w != m).any() for w, m in zip(want, masks))           # every tile's mask is cut: each copy-back shows
    src = [_dev(a) if k == 1 else a.copy() for k, a in enumerate(imgs)]
    mk = [_dev(m) if k == 1 else m.copy() for k, m in enumerate(masks)]
    assert gpu.GraphCutSeamFinder().find(src, corners, mk) is mk
    assert isinstance(mk[0], np.ndarray) and mk[1].is_cuda and isinstance(mk[2], np.ndarray)
    for k in range(3):
        assert np.array_equal(_np(mk[k]), want[k]), (k, int((_np(mk[k]) != want[k]).sum()))
        assert np.array_equal(_np(src[k]), imgs[k]), k


def test_growing_and_shrinking_sets_on_one_thread(gpu):
    """2, 5, then 2 host tiles through one finder on one thread (the staged copies of a tile index change size and count), then release()
    and one more call: every call equals the model."""
    f = gpu.GraphCutSeamFinder()
    for n, seed in [(2, 1), (5, 4), (2, 1), (0, 0), (3, 2)]:
        if n == 0:
            f.release()
            continue
        corners, imgs, masks = layout(n, seed)
        want = model(corners, imgs, masks)
        got = [m.copy() for m in masks]
        f.find([a.copy() for a in imgs], corners, got)
        for k in range(n):
            assert np.array_equal(got[k], want[k]), (n, k, int((got[k] != want[k]).sum()))
