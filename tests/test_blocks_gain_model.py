"""The NumPy model of BlocksGainCompensator (tests/helpers/blocks_gain_np.py, the spec of isx_blocks_gain_feed / isx_blocks_gain_apply) worked
by hand - the block grid, identical tiles, cv::resize's linear coefficients at the edges, the smoothing, hal::LU with row swaps - and the
CPU-side checks of the new entries: exported, declared, argument errors before any device call, and the library's host arithmetic (block
grids, the block pairs of two images by interval intersection, the smoothing, the resize tables: imagestitch_amd/csrc/blocks_gain_host.hpp)
built into a stand-alone program under AddressSanitizer and UBSan and compared with the model.  tests/test_gpu_blocks_gain.py compares the
GPU entries with the model."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blocks_gain_cases as cases  # noqa: E402
from helpers import blocks_gain_np as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the block grid ----------------------------------------------------------------------------------------------------------------------

def test_block_geometry_by_hand():
    assert M.block_grid(100, 80) == (4, 3, 25, 27)
    rects = M.block_rects(100, 80)
    assert len(rects) == 12 and rects[0] == (0, 0, 25, 27) and rects[3] == (75, 0, 25, 27)
    assert rects[8] == (0, 54, 25, 26) and rects[11] == (75, 54, 25, 26)          # the last row of blocks is 26 high
    assert M.block_grid(20, 9) == (1, 1, 20, 9) and M.block_rects(20, 9) == [(0, 0, 20, 9)]     # smaller than a block
    assert M.block_grid(7, 5, 1, 1) == (7, 5, 1, 1)                                # bl = 1: a map of the image's size
    assert M.block_grid(90, 70) == (3, 3, 30, 24) and M.block_rects(90, 70)[-1] == (60, 48, 30, 22)
    # blocks tile the image exactly, none empty, whatever the sizes
    for cols in range(1, 70):
        for bl in (1, 2, 3, 5, 7, 32):
            r = M.block_rects(cols, 1, bl, 1)
            assert r[0][0] == 0 and all(a[0] + a[2] == b[0] for a, b in zip(r, r[1:])) and r[-1][0] + r[-1][2] == cols
            assert all(a[2] >= 1 for a in r)


def test_block_corners_and_numbering():
    corners, imgs, masks = cases.two_tiles()
    bc, bi, _, owner, counts = M.split_blocks(corners, imgs, masks)
    assert counts == [(4, 3), (3, 3)] and owner == [0] * 12 + [1] * 9
    assert bc[5] == (25, 27) and bi[5].shape == (27, 25, 3)                        # by = 1, bx = 1 of tile 0
    assert bc[12] == (37, 5) and bc[12 + 4] == (67, 29) and bi[20].shape == (22, 30, 3)


# ---- feed --------------------------------------------------------------------------------------------------------------------------------

def test_identical_tiles_give_unit_gains_and_identity_apply():
    pano = np.random.default_rng(1).integers(0, 256, (120, 160, 3), dtype=np.uint8)
    corners = [(0, 0), (37, 5), (20, 40)]
    imgs = [pano[y:y + 70, x:x + 90] for x, y in corners]
    model = M.feed_blocks_model(corners, imgs, [np.full((70, 90), 255, np.uint8)] * 3)
    np.testing.assert_allclose(model["gains"], 1.0, rtol=0, atol=1e-12)
    ones = M.maps_from_gains(np.ones(27), model["counts"])
    for m in ones:
        assert np.array_equal(m, np.ones((3, 3), F32))                             # 0.5 + (1 + 1) 0.25 is exact
    for img, m in zip(imgs, ones):
        assert np.array_equal(M.apply_model(img, m), img)


def test_masks_with_holes_leave_pairs_without_a_counted_pixel():
    _, _, _, model = cases.case("two_tiles_holes")
    empty = [p for p in model["pairs"] if p[2] == 1 and p[3] == 0.0 and p[4] == 0.0]
    assert len(empty) == 6, empty                                                  # N = max(1, 0), I = 0
    assert len(model["pairs"]) == 25 and all(model["owner"][p[0]] == 0 and model["owner"][p[1]] == 1 for p in model["pairs"])
    _, _, _, three = cases.case("three_tiles")
    owners = {(three["owner"][p[0]], three["owner"][p[1]]) for p in three["pairs"]}
    assert owners == {(0, 1), (1, 2)}                                              # tiles 0 and 2 are apart


def test_sparse_system_is_the_dense_one():
    for name in list(cases.CASES) + list(cases.MORE):
        _, _, _, model = cases.case(name)
        r, c, v, b = M.sparse_system(model["pairs"], model["diag_n"])
        A = np.zeros_like(model["A"])
        A[r, c] = v
        assert np.array_equal(A, model["A"]) and np.array_equal(b, model["b"]), name


@pytest.mark.parametrize("name", sorted(cases.MORE))
def test_the_further_sets_reach_what_they_are_for(name):
    """cases.MORE: records of several work items (the second band shorter), a row wider than an item, no pair of blocks at all (every
    gain exactly 1.0), one-pixel blocks whose system swaps rows - from the geometry and gain.hip's constants; and the rtol of their gains."""
    cases.premise(name)
    rtol, measured = cases.gain_rtol(name)
    _, _, _, model = cases.case(name)
    print("%s: %d blocks, cond_1 %.3g, NumPy hal::LU against np.linalg.solve %.3g, rtol %.3g" % (name, len(model["b"]), np.linalg.cond(model["A"], 1), measured, rtol))
    assert 0 < len(model["b"]) * 2.0 ** -52 <= rtol / 4 <= 2.5e-10 and 4 * measured <= rtol


def test_bands_by_hand():
    assert cases.bands(150, 200, 16384) == [109, 91] and cases.bands(4097, 2, 4096) == [1, 1] and cases.bands(64, 64, 4096) == [64]
    assert cases.bands(113, 190, 4096) == [36] * 5 + [10] and cases.bands(1, 1, 4096) == [1] and cases.bands(4096, 3, 4096) == [1, 1, 1]
    diag, pairs = cases.record_items([(0, 0), (5, 0)], [(10, 10), (10, 10)], 32, 32, 16384, 4096)
    assert diag == [(10, 10, [10])] * 2 and pairs == [(5, 10, [10])]
    assert cases.record_items([(0, 0), (10, 0)], [(10, 10), (10, 10)], 4, 4, 16384, 4096)[1] == []           # they touch and do not meet


# ---- smoothing ---------------------------------------------------------------------------------------------------------------------------

def test_smoothing_by_hand():
    assert np.array_equal(M.smooth(np.array([[1.7]], F32)), np.array([[1.7]], F32) * F32(0.5) + (F32(1.7) + F32(1.7)) * F32(0.25))
    a, b, c = F32(1.0), F32(2.0), F32(4.0)
    # 1 x 3, one pass (the column pass of a single row gives x * 0.5 + (x + x) * 0.25 = x): REFLECT_101 mirrors b at both ends
    one = np.array([a * F32(.5) + (b + b) * F32(.25), b * F32(.5) + (a + c) * F32(.25), c * F32(.5) + (b + b) * F32(.25)], F32)
    assert list(one) == [1.5, 2.25, 3.0]
    two = np.array([one[0] * F32(.5) + (one[1] + one[1]) * F32(.25), one[1] * F32(.5) + (one[0] + one[2]) * F32(.25),
                    one[2] * F32(.5) + (one[1] + one[1]) * F32(.25)], F32)
    assert np.array_equal(M.smooth(np.array([[1, 2, 4]], F32)), two[None, :]) and list(two) == [1.875, 2.25, 2.625]
    assert np.array_equal(M.smooth(np.array([[1], [2], [4]], F32)), two[:, None])
    # 3 x 3 with one 16 in the middle: the row pass turns the middle row into 0 * 0.5 + (16 + 16) * 0.25 = 8, 16 * 0.5 + 0 = 8, 8 (REFLECT_101 counts
    # the middle twice from either end), the column pass every column [0, 8, 0] into 4, 4, 4; the second round leaves the constant 4
    m = np.zeros((3, 3), F32)
    m[1, 1] = 16
    assert np.array_equal(M.smooth(m), np.full((3, 3), 4, F32))
    # and a 3 x 3 ramp along x only: rows stay equal, each the 1 x 3 case
    assert np.array_equal(M.smooth(np.tile(np.array([1, 2, 4], F32), (3, 1))), np.tile(two, (3, 1)))


# ---- resize ------------------------------------------------------------------------------------------------------------------------------

def test_resize_columns_by_hand():
    a, b = F32(1.3), F32(2.9)
    got = M.resize_linear(np.array([[a, b]], F32), 4, 1)[0]
    want = [a, a * F32(.75) + b * F32(.25), a * F32(.25) + b * F32(.75), b]
    assert list(got) == want


def test_resize_rows_keep_their_fraction_at_the_edges():
    """3 rows to 7: fy(0) = (float)(0.5 * 3 / 7 - 0.5) < 0, sy = -1, fy -= sy gives about 0.714; both row indices clamp to 0, so the value is
    h * (1 - fy) + h * fy - which is not h for this h."""
    col = np.array([[1.9], [2.0], [3.0]], F32)
    got = M.resize_linear(col, 1, 7)[:, 0]
    fy = F32((0 + 0.5) * (1.0 / (7.0 / 3)) - 0.5)
    fy = F32(fy - F32(-1.0))
    h = F32(1.9)
    assert got[0] == F32(h * F32(F32(1) - fy) + h * fy)
    assert got[0] != h
    assert got[3] == F32(2.0)                                                      # the centre row falls on a source row
    fy6 = F32((6 + 0.5) * (1.0 / (7.0 / 3)) - 0.5)
    fy6 = F32(fy6 - F32(2.0))
    assert got[6] == F32(F32(3.0) * F32(F32(1) - fy6) + F32(3.0) * fy6)


def test_map_of_the_images_size_is_used_as_it_is():
    m = np.random.default_rng(3).random((5, 7)).astype(F32) + F32(0.5)
    assert M.gain_image(m, 7, 5) is m or np.array_equal(M.gain_image(m, 7, 5), m)
    assert not np.array_equal(M.resize_linear(m, 7, 6), m[:5])
    img = np.random.default_rng(4).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    want = np.clip(np.rint((img.astype(F32) * m[:, :, None]).astype(np.float64)), 0, 255).astype(np.uint8)
    assert np.array_equal(M.apply_model(img, m), want)


def test_apply_rounds_to_even_and_saturates():
    img = np.array([[[1, 3, 5], [200, 255, 0]]], np.uint8)
    assert M.apply_model(img, np.array([[0.5]], F32)).tolist() == [[[0, 2, 2], [100, 128, 0]]]
    assert M.apply_model(img, np.array([[1.5]], F32)).tolist() == [[[2, 4, 8], [255, 255, 0]]]
    assert M.apply_model(img, np.array([[-1.0]], F32)).tolist() == [[[0, 0, 0], [0, 0, 0]]]


# ---- hal::LU -----------------------------------------------------------------------------------------------------------------------------

def test_hal_lu_swaps_rows_and_agrees_with_numpy():
    _, _, _, model = cases.case("dark_against_bright")
    x, swaps = M.hal_lu_solve(model["A"], model["b"])
    assert swaps > 0
    np.testing.assert_allclose(x, np.linalg.solve(model["A"], model["b"]), rtol=1e-13, atol=0)
    assert M.hal_lu_solve(np.array([[0.0, 2.0], [4.0, 1.0]]), np.array([2.0, 6.0]))[1] == 1
    x, _ = M.hal_lu_solve(np.array([[0.0, 2.0], [4.0, 1.0]]), np.array([2.0, 6.0]))
    assert list(x) == [1.25, 1.0]
    assert M.hal_lu_solve(np.array([[1.0, 2.0], [2.0, 4.0]]), np.array([1.0, 2.0]))[0] is None      # singular
    # equal |values|: the first row wins (strict >)
    assert M.hal_lu_solve(np.array([[1.0, 2.0], [-1.0, 1.0]]), np.array([1.0, 1.0]))[1] == 0


# ---- the entries on the CPU side -----------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ["isx_blocks_gain_create", "isx_blocks_gain_destroy", "isx_blocks_gain_feed", "isx_blocks_gain_apply", "isx_blocks_gain_num_images",
               "isx_blocks_gain_block_counts", "isx_blocks_gain_gains", "isx_blocks_gain_map", "isx_blocks_gain_stats", "isx_blocks_gain_feed_times",
               "isx_selftest_lu_solve"]


def test_entries_are_exported_and_declared():
    from imagestitch_amd import _lib
    header = open(os.path.join(ROOT, "include", "imagestitch_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.declared_symbols(), name
        assert hasattr(lib, name), name
        assert "int %s(" % name in header, name
    assert "W:238-244" in header[header.index("typedef struct isx_blocks_gain"):header.index("isx_blocks_gain_feed_times")]
    import imagestitch_amd as I
    assert "BlocksGainCompensator" in I.__all__ and I.BlocksGainCompensator is not None
    mirror = open(os.path.join(ROOT, "include", "imagestitch.hpp")).read()
    assert "class BlocksGainCompensator" in mirror
    assert "class HipBlocksGainCompensator" in open(os.path.join(ROOT, "include", "imagestitch_cv_exposure.hpp")).read()


def test_argument_errors_come_before_any_device_call():
    import imagestitch_amd as I
    comp = I.BlocksGainCompensator()
    img = np.zeros((6, 9, 3), np.uint8)
    with pytest.raises(I.IsxError) as e:
        comp.apply(0, (0, 0), img)
    assert e.value.code == 3                                                       # apply before feed
    for query in (comp.gains, comp.gain_maps, comp.block_stats, comp.block_counts):
        with pytest.raises(I.IsxError) as e:
            query()
        assert e.value.code == 3
    with pytest.raises(I.IsxError) as e:
        comp.feed([], [], [])
    assert e.value.code == 1
    with pytest.raises(I.IsxError) as e:
        comp.feed([(0, 0)], [np.zeros((6, 9), np.uint8)], [np.full((6, 9), 255, np.uint8)])
    assert e.value.code == 2
    with pytest.raises(I.IsxError) as e:
        comp.feed([(0, 0)], [img], [np.full((6, 8), 255, np.uint8)])
    assert e.value.code == 7
    with pytest.raises(I.IsxError) as e:
        I.BlocksGainCompensator(0, 32)
    assert e.value.code == 1
    # 129 x 128 blocks of one pixel: 16 512 unknowns, more than the 16 384 of a 2 GiB matrix
    big = np.zeros((128, 129, 3), np.uint8)
    with pytest.raises(I.IsxError) as e:
        I.BlocksGainCompensator(1, 1).feed([(0, 0)], [big], [np.full((128, 129), 255, np.uint8)])
    assert e.value.code == 6


def test_feed_without_a_gpu_is_a_hip_error():
    """No CPU fallback: on a box without a GPU feed fails with ISX_ERR_HIP; with one it runs."""
    import torch
    import imagestitch_amd as I
    corners, imgs, masks = cases.two_tiles()
    comp = I.BlocksGainCompensator()
    if torch.cuda.is_available():
        assert comp.feed(corners, imgs, masks).gains().size == 21
        return
    with pytest.raises(I.IsxError) as e:
        comp.feed(corners, imgs, masks)
    assert e.value.code == 4
    with pytest.raises(I.IsxError) as e:
        from imagestitch_amd import exposure
        exposure.lu_solve(np.eye(2), np.ones(2))
    assert e.value.code == 4


# ---- the library's host arithmetic under the sanitizers --------------------------------------------------------------------------------------

def _hex(v):
    return float(v).hex()


def test_host_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "blocks_gain_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "blocks_gain_host.cpp"),
                           "-o", exe])
    rng = np.random.default_rng(11)
    grids = [(100, 80, 32, 32), (90, 70, 32, 32), (20, 9, 32, 32), (7, 5, 1, 1), (1101, 1101, 32, 32), (3840, 2160, 64, 64), (33, 65, 32, 32), (1, 1, 5, 3)]
    pairs = [(0, 0, 100, 80, 37, 5, 90, 70, 32, 32), (0, 0, 100, 80, 99, 79, 90, 70, 32, 32), (0, 0, 100, 80, 100, 0, 90, 70, 32, 32),
             (-30, -20, 55, 41, -12, -33, 47, 36, 8, 5), (2**31 - 60, 2**31 - 50, 50, 40, 2**31 - 40, 2**31 - 70, 30, 60, 7, 7),
             (-2**31, -2**31, 64, 64, -2**31 + 13, -2**31 + 40, 90, 30, 16, 9), (5, 5, 10, 10, 0, 0, 60, 60, 4, 4), (0, 0, 37, 29, 0, 0, 37, 29, 5, 3),
             # blocks larger than the images, a block wider than a work item, one-pixel blocks (the sets of cases.MORE)
             (0, 0, 300, 200, 37, 5, 280, 190, 200, 200), (0, 0, 4100, 3, -3, 1, 4100, 4, 8192, 32), (0, 0, 9, 7, 4, 3, 8, 6, 1, 1),
             (0, 0, 40, 30, 100, 100, 20, 20, 32, 32)]
    smooths = [rng.random((ny, nx)).astype(F32) + F32(0.5) for ny, nx in ((1, 1), (1, 3), (3, 3), (1, 2), (2, 1), (5, 7), (34, 3))]
    tables = [(2, 1, 4, 1), (1, 3, 1, 7), (3, 2, 67, 45), (1, 1, 9, 9), (4, 3, 3, 2), (35, 35, 1101, 1101), (7, 5, 8, 6), (60, 34, 3840, 2160),
              (13, 7, 5, 7), (13, 7, 13, 3), (13, 7, 4, 3), (13, 7, 40, 3), (1, 5, 20, 40), (5, 1, 257, 17)]      # a map larger than the image, one block wide, one block high
    text = "".join("grid %d %d %d %d\n" % g for g in grids) + "".join("pairs " + " ".join(str(v) for v in p) + "\n" for p in pairs)
    text += "".join("smooth %d %d %s\n" % (m.shape[0], m.shape[1], " ".join(_hex(v) for v in m.ravel())) for m in smooths)
    text += "".join("tables %d %d %d %d\n" % t for t in tables)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(grids) + len(pairs) + len(smooths) + len(tables)
    it = iter(lines)
    for cols, rows, blw, blh in grids:
        t = [int(v) for v in next(it).split()]
        assert tuple(t[:4]) == M.block_grid(cols, rows, blw, blh)
        assert [tuple(t[4 + 4 * k:8 + 4 * k]) for k in range((len(t) - 4) // 4)] == M.block_rects(cols, rows, blw, blh)
    met = 0
    for xi, yi, wi, hi, xj, yj, wj, hj, blw, blh in pairs:
        t = [int(v) for v in next(it).split()]
        got = [tuple(t[1 + 8 * k:9 + 8 * k]) for k in range(t[0])]
        # every pair of blocks, all against all, on Python integers
        ri, rj = M.block_rects(wi, hi, blw, blh), M.block_rects(wj, hj, blw, blh)
        want = []
        for a, (ax, ay, aw, ah) in enumerate(ri):
            for b, (bx, by, bw, bh) in enumerate(rj):
                x0, y0 = max(xi + ax, xj + bx), max(yi + ay, yj + by)
                x1, y1 = min(xi + ax + aw, xj + bx + bw), min(yi + ay + ah, yj + by + bh)
                if x0 < x1 and y0 < y1:
                    want.append((a, len(ri) + b, x0 - xi, y0 - yi, x0 - xj, y0 - yj, x1 - x0, y1 - y0))
        assert got == want, (xi, yi, xj, yj)
        met += len(want)
    assert met > 40
    for m in smooths:
        got = np.array([float.fromhex(v) for v in next(it).split()], F32).reshape(m.shape)
        assert np.array_equal(got, M.smooth(m))
    for sw, sh, dw, dh in tables:
        t = next(it).split()
        sx, fx = M.resize_taps(sw, dw)
        fx = np.where((sx < 0) | (sx >= sw - 1), F32(0), fx)
        sx = np.clip(sx, 0, sw - 1)
        sy, fy = M.resize_taps(sh, dh)
        want = []
        for a, f in zip(sx, fx):
            want += [str(int(a)), _hex(f)]
        for a, f in zip(sy, fy):
            want += [str(int(np.clip(a, 0, sh - 1))), str(int(np.clip(a + 1, 0, sh - 1))), _hex(f)]
        assert [v if not v.startswith(("0x", "-0x")) else float.fromhex(v).hex() for v in t] == want, (sw, sh, dw, dh)
