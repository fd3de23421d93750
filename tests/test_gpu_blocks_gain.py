"""BlocksGainCompensator on the GPU (isx_blocks_gain_feed / isx_blocks_gain_apply) against the NumPy model of tests/helpers/blocks_gain_np.py:
the sparse statistics exactly (N) and bit for bit (I), the gains against np.linalg.solve on the model's system, the solver alone, a
2 450-unknown system by its residual, the smoothed maps and apply bit for bit, guard bands, the call surface (errors, capture, graph replay,
feeding twice), warp -> feed -> apply against the oracle, and the C++ mirror and OpenCV adapter.

Tolerances.  The device runs hal::LU's elimination operation for operation; only the additions of its back substitution are ordered
otherwise.  rtol of the gains = 4 x the largest relative difference between np.linalg.solve and the NumPy hal::LU over the cases used, at
most 1e-9 - computed by the tests, on the CPU.  Measured on the CPU: 1.03e-15 over the four tile sets of tests/blocks_gain_cases.py (21 and
18 blocks, condition numbers 9 to 37; rtol 4.1e-15), 6 row swaps in "dark_against_bright"; 1.4e-13 over the dense systems of the solver's
own test (rtol 5.6e-13).  The 2 450-unknown system: scipy.sparse.linalg.spsolve leaves ||A g - b||inf / (||A||inf ||g||inf + ||b||inf) =
1.5e-16 (computed by the test from the library's statistics, printed with the library's own figure); the bound is 8 x that."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blocks_gain_cases as cases  # noqa: E402
from helpers import blocks_gain_np as M  # noqa: E402
from helpers import guarded  # noqa: E402
from imagestitch_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_UNSUPPORTED, ERR_INTERNAL = 1, 2, 3, 6, 9


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


@functools.lru_cache(maxsize=None)
def _gain_rtol():
    """4 x the largest relative difference between np.linalg.solve and the NumPy hal::LU over the tile sets, at most 1e-9."""
    worst = max(cases.lu_rel_diff(name)[0] for name in cases.CASES)
    assert 0 < worst < 1e-13
    return min(4 * worst, 1e-9)


def _check_stats(comp, model):
    assert comp.block_counts() == model["counts"]
    pairs, diag = comp.block_stats()
    assert np.array_equal(diag, model["diag_n"])
    want = model["pairs"]
    assert len(pairs) == len(want)
    assert [(int(p["block_i"]), int(p["block_j"]), int(p["n"])) for p in pairs] == [p[:3] for p in want]
    assert np.array_equal(pairs["i_ij"].view(np.uint64), np.array([p[3] for p in want]).view(np.uint64))
    assert np.array_equal(pairs["i_ji"].view(np.uint64), np.array([p[4] for p in want]).view(np.uint64))


def _check(gpu, name, images=None, masks=None):
    corners, imgs, msks, model = cases.case(name)
    comp = gpu.BlocksGainCompensator().feed(corners, imgs if images is None else images, msks if masks is None else masks)
    _check_stats(comp, model)
    g = comp.gains()
    print("%s: largest relative difference of the gains to np.linalg.solve %.3g (rtol %.3g)" % (name, np.max(np.abs(g - model["gains"]) / np.abs(model["gains"])), _gain_rtol()))
    np.testing.assert_allclose(g, model["gains"], rtol=_gain_rtol(), atol=0)
    maps = comp.gain_maps()
    for got, want in zip(maps, M.maps_from_gains(g, model["counts"])):
        assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return comp


# ---- statistics, gains, maps ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_statistics_gains_and_maps(gpu, name, where):
    corners, imgs, masks, model = cases.case(name)
    if name == "two_tiles_holes":
        assert sum(1 for p in model["pairs"] if p[2] == 1 and p[3] == 0.0) == 6
    if name == "dark_against_bright":
        assert cases.lu_rel_diff(name)[1] > 0                      # the model's hal::LU swaps rows: the case exercises pivoting
        assert len(model["diag_n"]) == 21
    if where == "device":
        imgs, masks = [_dev(a) for a in imgs], [_dev(m) for m in masks]
    _check(gpu, name, imgs, masks)


@pytest.mark.parametrize("where", ["host", "device"])
def test_pitched_unaligned_views_and_feed_writes_nothing(gpu, where):
    """Views into larger buffers (tests/helpers/guarded.py), odd and aligned layouts mixed image against mask, 255 all around the masks (a mask
    read past its view would count): the model's statistics, and not one byte of the buffers written."""
    corners, imgs, masks, _ = cases.case("two_tiles_holes")
    odd, aligned = guarded.LAYOUTS
    for p, (li, lm) in enumerate(((odd, odd), (aligned, odd), (odd, aligned))):
        gi = [guarded.guarded_like(a, where, li if k == 0 else lm, 10 * p + k) for k, a in enumerate(imgs)]
        gm = [guarded.guarded_like(m, where, lm if k == 0 else li, 10 * p + 5 + k) for k, m in enumerate(masks)]
        for g, m in zip(gm, masks):
            g.buf[...] = 255
            g.set(m)
        _check(gpu, "two_tiles_holes", [g.view for g in gi], [g.view for g in gm])
        for g in gi + gm:
            g.check(guarded.NOTHING)


def test_feeding_twice_gives_the_second_sets_results(gpu):
    corners, imgs, masks, model = cases.case("three_tiles")
    comp = gpu.BlocksGainCompensator().feed(*cases.case("dark_against_bright")[:3])
    assert comp.gains().size == 21
    comp.feed(corners, imgs, masks)
    _check_stats(comp, model)
    np.testing.assert_allclose(comp.gains(), model["gains"], rtol=_gain_rtol(), atol=0)
    assert len(comp.gain_maps()) == 3


# ---- the solver alone ----------------------------------------------------------------------------------------------------------------------

def _dense(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) + np.diag(rng.uniform(1, 2, n) * np.sqrt(n))
    return A, rng.uniform(1, 2, n)


def _pivot_in_last_row(n=21):
    A, b = _dense(n, 77)
    A[-1, 0] = 50.0                                                # column 0's largest |value| sits in the last row
    return A, b


def _swap_at_every_step(n=21):
    """A cyclic shift of a dominant diagonal: the largest |value| of every column lies below the diagonal until the last."""
    rng = np.random.default_rng(78)
    A = 0.01 * rng.standard_normal((n, n))
    for c in range(n):
        A[(c + 1) % n, c] = 10.0 + c
    return A, rng.uniform(1, 2, n)


@functools.lru_cache(maxsize=None)
def _systems():
    out = {"n%d" % n: _dense(n, 100 + n) for n in (1, 2, 21, 67, 257)}
    out["pivot_in_last_row"] = _pivot_in_last_row()
    out["swap_at_every_step"] = _swap_at_every_step()
    ref = {}
    for k, (A, b) in out.items():
        x, swaps = M.hal_lu_solve(A, b)
        want = np.linalg.solve(A, b)
        ref[k] = (want, swaps, float(np.max(np.abs(x - want) / np.abs(want))))
    return out, ref, min(4 * max(r[2] for r in ref.values()), 1e-9)


def test_solver_alone(gpu):
    from imagestitch_amd import exposure
    systems, ref, rtol = _systems()
    assert 0 < rtol <= 1e-9
    assert ref["pivot_in_last_row"][1] >= 1 and ref["swap_at_every_step"][1] == 20
    for k, (A, b) in systems.items():
        x, swaps = exposure.lu_solve(A, b)
        want, model_swaps, _ = ref[k]
        print("%s: swaps %d, largest relative difference to np.linalg.solve %.3g (rtol %.3g)" % (k, swaps, np.max(np.abs(x - want) / np.abs(want)), rtol))
        assert swaps == model_swaps, k
        np.testing.assert_allclose(x, want, rtol=rtol, atol=0, err_msg=k)
        xh, _ = exposure.lu_solve(A, b, where="host")
        np.testing.assert_allclose(xh, want, rtol=rtol, atol=0, err_msg=k)


def test_singular_matrix_is_an_error_and_everything_stays_usable(gpu):
    from imagestitch_amd import exposure
    comp = _check(gpu, "three_tiles")
    A = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 0.0, 1.0]])
    with pytest.raises(gpu.IsxError) as e:
        exposure.lu_solve(A, np.ones(3))
    assert e.value.code == ERR_INTERNAL and "singular" in e.value.msg
    with pytest.raises(gpu.IsxError) as e:
        exposure.lu_solve(np.zeros((5, 5)), np.ones(5))
    assert e.value.code == ERR_INTERNAL
    x, _ = exposure.lu_solve(np.array([[2.0, 0.0], [0.0, 4.0]]), np.array([2.0, 2.0]))
    assert list(x) == [1.0, 0.5]
    img = cases.case("three_tiles")[1][0].copy()
    want = M.apply_model(img, comp.gain_maps()[0])
    assert np.array_equal(comp.apply(0, (0, 0), img), want)        # the handle fed before still applies
    _check(gpu, "three_tiles")


# ---- a large system, no dense model ----------------------------------------------------------------------------------------------------------

def test_large_system_by_its_residual(gpu):
    """Two 1101 x 1101 tiles at the reference's offset (dx = 799), 32 x 32 blocks: 2 450 unknowns.  The sparse system is rebuilt from
    block_stats(); the library's gains must leave a residual within 8 x that of scipy's sparse direct solve."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import torch
    rng = np.random.default_rng(5)
    base = rng.integers(0, 200, (1101, 1101 + 799, 3), dtype=np.uint8)
    t0 = base[:, :1101]
    t1 = np.clip(base[:, 799:].astype(np.int32) * 5 // 4 + 10, 0, 255).astype(np.uint8)      # the same scene, exposed otherwise
    mask = torch.full((1101, 1101), 255, dtype=torch.uint8, device="cuda")
    comp = gpu.BlocksGainCompensator().feed([(0, 0), (799, 0)], [_dev(t0), _dev(t1)], [mask, mask])
    assert comp.block_counts() == [(35, 35), (35, 35)]
    g = comp.gains()
    assert g.size == 2450
    pairs, diag = comp.block_stats()
    assert len(pairs) == 700 and diag.max() == 32 * 32 and diag.min() == 13 * 13          # 34 blocks of 32 and one of 13 each way; 10 x 35 blocks of tile 0 meet 2 each
    r, c, v, b = M.sparse_system([tuple(p) for p in pairs.tolist()], diag)
    A = sp.csr_matrix((v, (r, c)), shape=(2450, 2450))
    ninf = abs(A).sum(axis=1).max()

    def ratio(x):
        return float(np.max(np.abs(A @ x - b)) / (ninf * np.max(np.abs(x)) + np.max(np.abs(b))))
    ref = ratio(spl.spsolve(A.tocsc(), b))
    got = ratio(g)
    print("residual ratio: library %.3g, spsolve %.3g (bound 8 x)" % (got, ref))
    assert ref > 0 and got <= 8 * ref
    # neither all ones nor all zeros: the tiles differ in exposure, and the blocks on the overlap pull apart
    assert g.min() > 0.5 and g.max() < 1.5 and g.max() - g.min() > 0.1
    assert g[:1225].mean() > 1.0 > g[1225:].mean()
    print("feed stages, ms:", comp.feed_times())


# ---- apply ---------------------------------------------------------------------------------------------------------------------------------

APPLY = {                     # name: (width, height, bl_width, bl_height)
    "map_3x2": (67, 45, 32, 32),                  # 16 groups of four pixels and a partial one
    "past_a_workgroup": (261, 19, 32, 32),        # a workgroup spans 256 columns and 16 rows: a second one each way, and a partial group
    "map_1x1": (20, 9, 32, 32),
    "map_of_the_images_size": (13, 7, 1, 1),
    "tall_blocks": (40, 70, 8, 64),
}


@functools.lru_cache(maxsize=None)
def _fed(name):
    """A compensator fed with a dark and a bright tile of the case's size (gains up to about 2 and down to about 0.5), its maps, and the
    dark tile with a bright corner that its gains saturate."""
    import imagestitch_amd as gpu
    w, h, blw, blh = APPLY[name]
    rng = np.random.default_rng(len(name))
    imgs = [rng.integers(60, 120, (h, w, 3), dtype=np.uint8), rng.integers(150, 256, (h, w, 3), dtype=np.uint8)]
    masks = [np.full((h, w), 255, np.uint8)] * 2
    comp = gpu.BlocksGainCompensator(blw, blh).feed([(0, 0), (w // 3, h // 4)], imgs, masks)
    maps = comp.gain_maps()
    assert maps[0].shape == M.block_grid(w, h, blw, blh)[1::-1] and maps[0].max() > 1.05 and maps[1].min() < 0.95
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return comp, maps, img


@pytest.mark.parametrize("where", ["host", "device", "host_odd", "device_odd", "device_aligned"])
@pytest.mark.parametrize("name", sorted(APPLY))
def test_apply(gpu, name, where):
    """Bit for bit the model's apply on the library's own maps; in a guard band, the image's bytes and nothing beside them."""
    comp, maps, img = _fed(name)
    for index in (0, 1):
        want = M.apply_model(img, maps[index])
        if index == 0:
            assert np.any((img.astype(F32) * M.gain_image(maps[0], img.shape[1], img.shape[0])[:, :, None]) > 255.5)      # saturates at 255
            assert want.max() == 255 and not np.array_equal(want, img)
        if where == "host":
            a = img.copy()
            assert comp.apply(index, (0, 0), a) is a and np.array_equal(a, want)
        elif where == "device":
            t = _dev(img)
            comp.apply(index, (0, 0), t, None)
            assert np.array_equal(_np(t), want)
        else:
            place, layout = where.split("_")
            g = guarded.guarded_like(img, place, layout, 3 + index)
            comp.apply(index, (0, 0), g.view)
            if place == "device":
                import torch
                torch.cuda.synchronize()
            g.check()
            assert np.array_equal(g.get(), want)


def test_apply_on_an_image_of_another_size(gpu):
    """OpenCV resizes the map to whatever image it is given; so does this.  Also a size that makes the map the image's size by accident."""
    comp, maps, _ = _fed("map_3x2")
    rng = np.random.default_rng(9)
    for w, h in ((50, 31), (3, 2), (1, 1), (130, 7), (5, 300)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        t = _dev(img)
        comp.apply(1, (0, 0), t)
        assert np.array_equal(_np(t), M.apply_model(img, maps[1])), (w, h)
    assert np.array_equal(M.gain_image(maps[1], 3, 2), maps[1])


# ---- the call surface ------------------------------------------------------------------------------------------------------------------------

def test_errors(gpu):
    comp = gpu.BlocksGainCompensator()
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(gpu.IsxError) as e:
        comp.apply(0, (0, 0), _dev(img))
    assert e.value.code == ERR_STATE
    comp, _, _ = _fed("map_1x1")
    for index in (-1, 2):
        with pytest.raises(gpu.IsxError) as e:
            comp.apply(index, (0, 0), _dev(img))
        assert e.value.code == ERR_INVALID
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.int16)):
        with pytest.raises(gpu.IsxError) as e:
            comp.apply(0, (0, 0), _dev(bad))
        assert e.value.code == ERR_TYPE
    big = _dev(np.zeros((128, 129, 3), np.uint8))                  # 16 512 blocks of one pixel
    with pytest.raises(gpu.IsxError) as e:
        gpu.BlocksGainCompensator(1, 1).feed([(0, 0)], [big], [_dev(np.full((128, 129), 255, np.uint8))])
    assert e.value.code == ERR_UNSUPPORTED
    t = _dev(img + 100)
    comp.apply(0, (0, 0), t)                                       # still usable
    assert np.array_equal(_np(t), M.apply_model(img + 100, comp.gain_maps()[0]))


def test_feed_refuses_a_capturing_stream_and_apply_is_captured_and_replayed(gpu):
    import torch
    corners, imgs, masks, model = cases.case("two_tiles")
    s = torch.cuda.Stream()
    comp = gpu.BlocksGainCompensator(stream=s)
    with torch.cuda.stream(s):
        dimgs, dmasks = [_dev(a) for a in imgs], [_dev(m) for m in masks]
        x = torch.zeros(16, device="cuda")
        comp.feed(corners, dimgs, dmasks)
        tile = _dev(imgs[0])
        other = torch.zeros((31, 50, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    maps = comp.gain_maps()
    gains = comp.gains()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(gpu.IsxError) as e:
            comp.feed(corners, dimgs, dmasks)
        assert e.value.code == ERR_STATE and "captur" in e.value.msg
        with pytest.raises(gpu.IsxError) as e:                     # a size whose tables are not built yet
            comp.apply(0, corners[0], other)
        assert e.value.code == ERR_STATE and "captur" in e.value.msg
        comp.apply(0, corners[0], tile)                            # the size fed: captured
    torch.cuda.synchronize()
    assert float(x[0]) == 0.0 and np.array_equal(_np(tile), imgs[0])                # captured, not run; the capture is intact
    assert np.array_equal(comp.gains(), gains)                     # the refused feed left the handle as it was
    want = imgs[0]
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        want = M.apply_model(want, maps[0])
        assert float(x[0]) == k + 1.0 and np.array_equal(_np(tile), want), k


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_warp_feed_apply(gpu, oracle):
    """W:229-244 on a reduced config-2 pair (a quarter of 4K, 64 x 64 blocks: about 270 unknowns): warp, feed, apply on the GPU, byte for byte the
    oracle's warp run through the model."""
    import torch
    W, H, F = 960, 540, 750.0
    K, Rs = synth.camera_pair(W, H, F)
    srcs = [synth.make_tile(H, W, 30 + i) for i in range(2)]
    srcs[0] = (srcs[0] // 2 + 20).astype(np.uint8)
    warper = gpu.CylindricalWarper().create(F)
    corners, wis, wms, o_wis, o_wms = [], [], [], [], []
    for i in range(2):
        c, wi, wm = warper.warp_with_mask(torch.from_numpy(srcs[i]).cuda(), K, Rs[i])
        oc, owi, _ = oracle.warp_u8(oracle.CYL, F, K, Rs[i], srcs[i], oracle.LINEAR, oracle.BORDER_REFLECT)
        _, owm, _ = oracle.warp_u8(oracle.CYL, F, K, Rs[i], np.full((H, W), 255, np.uint8), oracle.NEAREST, oracle.BORDER_CONSTANT)
        assert oc == c
        corners.append(c); wis.append(wi); wms.append(wm); o_wis.append(owi); o_wms.append(owm)
    comp = gpu.BlocksGainCompensator(64, 64).feed(corners, wis, wms)
    model = M.feed_blocks_model(corners, o_wis, o_wms, 64, 64)
    assert 200 < len(model["diag_n"]) < 400
    _check_stats(comp, model)
    x, _ = M.hal_lu_solve(model["A"], model["b"])
    rtol = min(4 * float(np.max(np.abs(x - model["gains"]) / np.abs(model["gains"]))), 1e-9)
    np.testing.assert_allclose(comp.gains(), model["gains"], rtol=rtol, atol=0)
    maps = comp.gain_maps()
    assert maps[0].mean() > 1.0
    for i in range(2):
        comp.apply(i, corners[i], wis[i], wms[i])
        assert np.array_equal(wis[i].cpu().numpy(), M.apply_model(o_wis[i], maps[i])), i


# ---- the C++ mirror and the OpenCV adapter -----------------------------------------------------------------------------------------------------

def test_cpp_blocks_gain_demo(gpu, tmp_path):
    """isx::BlocksGainCompensator (include/imagestitch.hpp) and HipBlocksGainCompensator through cv::detail::ExposureCompensator
    (include/imagestitch_cv_exposure.hpp, compiled against tests/cpp/opencv_stub with -Werror=suggest-override) against the model."""
    exe = str(tmp_path / "blocks_gain_demo")
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Wsuggest-override", "-Woverloaded-virtual", "-Werror=suggest-override",
                           "-Werror=overloaded-virtual", "-I", os.path.join(ROOT, "tests", "cpp", "opencv_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "blocks_gain_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
    corners, imgs, masks, model = cases.case("two_tiles_holes")
    for k in range(2):
        imgs[k].tofile(str(tmp_path / ("img%d.raw" % k)))
        masks[k].tofile(str(tmp_path / ("mask%d.raw" % k)))
    args = [exe, str(tmp_path), "2"] + ["%d %d %d %d" % (c[0], c[1], m.shape[1], m.shape[0]) for c, m in zip(corners, masks)]
    out = subprocess.check_output(" ".join(args).split(), text=True, timeout=300)
    got = {}
    for line in out.splitlines():
        t = line.split()
        if t and t[0] in ("mirror", "adapter"):
            got[t[0]] = np.array([float.fromhex(x) for x in t[1:]])
    for leg in ("mirror", "adapter"):
        np.testing.assert_allclose(got[leg], model["gains"], rtol=_gain_rtol(), atol=0)
    assert np.array_equal(got["mirror"], got["adapter"])
    # the demo writes what apply() made of every tile: the model's apply on the maps of the gains it printed
    maps = M.maps_from_gains(got["adapter"], model["counts"])
    for k in range(2):
        for leg in ("mirror", "adapter"):
            applied = np.fromfile(str(tmp_path / ("%s%d.raw" % (leg, k))), np.uint8).reshape(imgs[k].shape)
            assert np.array_equal(applied, M.apply_model(imgs[k], maps[k])), (leg, k)
    assert "throws 3" in out and "throws 7" in out
