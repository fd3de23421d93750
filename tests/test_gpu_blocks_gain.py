"""BlocksGainCompensator on the GPU (isx_blocks_gain_feed / isx_blocks_gain_apply) against the NumPy model of tests/helpers/blocks_gain_np.py:
the sparse statistics exactly (N) and bit for bit (I), the gains against np.linalg.solve on the model's system, the solver alone, a
2 450-unknown system by its residual, the smoothed maps and apply bit for bit, guard bands, the call surface (errors, capture, graph replay,
feeding twice), warp -> feed -> apply against the oracle, and the C++ mirror and OpenCV adapter.

Tolerances.  The device runs hal::LU's elimination operation for operation; only the additions of its back substitution are ordered
otherwise.  rtol of the gains = 4 x the largest relative difference between np.linalg.solve and the NumPy hal::LU over the cases used, at
most 1e-9 - computed by the tests, on the CPU.  Measured on the CPU: 1.03e-15 over the four tile sets of tests/blocks_gain_cases.py (21 and
18 blocks, condition numbers 9 to 37; rtol 4.1e-15), 6 row swaps in "dark_against_bright"; 1.4e-13 over the dense systems of the solver's
own test (rtol 5.6e-13).  The 2 450-unknown system: scipy.sparse.linalg.spsolve leaves ||A g - b||inf / (||A||inf ||g||inf + ||b||inf) =
1.5e-16 (computed by the test from the library's statistics, printed with the library's own figure); the bound is 8 x that.

The sets of cases.MORE (three tiles that all meet, records of several work items, a row wider than an item, no pair at all, one-pixel
blocks) have a rtol of their own: on several of them the two CPU solves agree to the last bit, and rtol 0 is no fair demand of a back
substitution that adds in another order.  Per set rtol = min(1e-9, 4 max(that difference, B 2^-52 cond_1(A))), A the model's dense system
(cases.forward_error_rtol): the textbook forward-error scale, from the model alone.  Measured on the CPU: differences 0 to 2.2e-16,
rtol 4.3e-15 ("apart", 3 blocks, cond 1.6) to 4.3e-12 ("one_pixel_blocks", 111 blocks, cond 44, 20 row swaps).  The solver past one stride
of its pivot search (n = 513, 1025, 1100): the model's differences are 6.8e-15 to 1.7e-12, its swaps 0, 1, 2, 2 and 0."""
import functools
import gc
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
    """The sets of cases.CASES keep their rtol (_gain_rtol); a set of cases.MORE has its own, cases.gain_rtol."""
    corners, imgs, msks, model = cases.case(name)
    comp = gpu.BlocksGainCompensator(*cases.blocks(name)).feed(corners, imgs if images is None else images, msks if masks is None else masks)
    _check_stats(comp, model)
    g = comp.gains()
    rtol = _gain_rtol() if name in cases.CASES else cases.gain_rtol(name)[0]
    print("%s: largest relative difference of the gains to np.linalg.solve %.3g (rtol %.3g)" % (name, np.max(np.abs(g - model["gains"]) / np.abs(model["gains"])), rtol))
    np.testing.assert_allclose(g, model["gains"], rtol=rtol, atol=0)
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


# ---- records of several work items, a row wider than an item, no pair at all, one-pixel blocks -------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device", "host_odd", "device_odd"])
@pytest.mark.parametrize("name", sorted(cases.MORE))
def test_more_sets(gpu, name, where):
    """The sets of cases.MORE through _check (block counts, N exactly, I bit for bit, gains, maps bit for bit), then apply on every tile: as
    host mats, as device mats, and as pitched unaligned views in guard bands with 255 all around the masks - feed writes nothing, apply
    the image's bytes only.  Without a pair of blocks that meet every gain is exactly 1.0 and apply leaves the image byte for byte."""
    import torch
    corners, imgs, masks, model = cases.case(name)
    cases.premise(name)
    gi = gm = None
    if where == "host":
        mi, mm = [a.copy() for a in imgs], [m.copy() for m in masks]
    elif where == "device":
        mi, mm = [_dev(a) for a in imgs], [_dev(m) for m in masks]
    else:
        place = where.split("_")[0]
        gi = [guarded.guarded_like(a, place, "odd", 20 + k) for k, a in enumerate(imgs)]
        gm = [guarded.guarded_like(m, place, "odd", 30 + k) for k, m in enumerate(masks)]
        for g, m in zip(gm, masks):
            g.buf[...] = 255
            g.set(m)
        mi, mm = [g.view for g in gi], [g.view for g in gm]
    comp = _check(gpu, name, mi, mm)
    if gi:
        for g in gi + gm:
            g.check(guarded.NOTHING)
    g = comp.gains()
    maps = comp.gain_maps()
    if name in cases.NO_PAIRS:
        assert len(comp.block_stats()[0]) == 0
        assert np.all(g == 1.0) and all(np.all(m == F32(1)) for m in maps)
    for k, img in enumerate(imgs):
        want = M.apply_model(img, maps[k])
        if name in cases.NO_PAIRS:
            assert np.array_equal(want, img)
        comp.apply(k, corners[k], mi[k], mm[k])
        torch.cuda.synchronize()
        assert np.array_equal(_np(mi[k]), want), k
        if gi:
            gi[k].check()
            gm[k].check(guarded.NOTHING)


def test_map_query_into_pitched_mats(gpu):
    """isx_blocks_gain_map itself, on the handle's stream: into pitched host mats (row by row) and into pitched device mats (one
    hipMemcpy2DAsync with the caller's pitch), both layouts, inside guard bands: gain_maps() bit for bit and nothing written beside it."""
    import ctypes as C
    import torch
    from imagestitch_amd import _lib
    corners, imgs, masks, _ = cases.case("three_tiles")
    s = torch.cuda.Stream()
    comp = gpu.BlocksGainCompensator(stream=s).feed(corners, imgs, masks)
    maps = comp.gain_maps()
    assert [m.shape for m in maps] == [(2, 3), (2, 3), (3, 2)]
    lib = _lib.load()
    for where in ("host", "device"):
        for layout in guarded.LAYOUTS:
            for i, m in enumerate(maps):
                g = guarded.guarded_like(np.zeros_like(m), where, layout, 50 + i)
                mm = _lib.as_mat(g.view)
                assert mm.step > m.shape[1] * 4
                _lib.check(lib.isx_blocks_gain_map(comp._h, i, C.byref(mm), comp._stream()))
                torch.cuda.synchronize()
                g.check()
                assert np.array_equal(g.get().view(np.uint32), m.view(np.uint32)), (where, layout, i)


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


def _lu_constants():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity
    c = fuzz_parity._kernel_consts("blocks_gain.hip")
    return c["LU_PNT"], c["LU_NT"]


def _dominant(n, seed):
    """A diagonal in [4, 5] over off-diagonal noise of 0.01 x normal: hal::LU swaps no rows until an entry is planted."""
    rng = np.random.default_rng(seed)
    A = 0.01 * rng.standard_normal((n, n))
    A[np.arange(n), np.arange(n)] = rng.uniform(4, 5, n)
    return A, rng.uniform(1, 2, n)


def _planted(n, seed, entries):
    A, b = _dominant(n, seed)
    for (r, c), v in entries.items():
        A[r, c] = v
    return A, b


def _pivot_in_the_second_stride():
    """n = LU_PNT + 1: row LU_PNT is the only one k_lu_pivot's second stride holds, and column 0's largest |value| sits there."""
    n = _lu_constants()[0] + 1
    A, b = _dense(n, 100 + n)
    A[n - 1, 0] = 2.0 * np.abs(A[:, 0]).max()
    return A, b


# n = 1100 is past LU_PNT = 1024: rows 1024.. are the pivot search's second stride, and k_lu_backsub's dot products take two strides.
# "tie_diagonal" and "tie_below": column 0 is searched before anything is eliminated, so its tie is exact.  In the first the diagonal is
# among the tied rows (0, 70 and 1030) and, being the first of them, is the pivot: no swap there.  In the second the diagonal is smaller
# than the tied rows (70, 200 and 1030): a swap there.  The two tell "the first of the tied rows when that is the diagonal" from any
# other choice; which of two tied rows BELOW the diagonal is taken shows neither in x nor in the swap count, and nothing here claims it.
LARGE = {
    "pivot_in_the_second_stride": _pivot_in_the_second_stride,
    "pivots_past_one_stride": lambda: _planted(1100, 79, {(1050, 0): 50.0, (1099, 3): -60.0}),
    "tie_diagonal": lambda: _planted(1100, 80, {(0, 0): 5.0, (70, 0): -5.0, (1030, 0): 5.0}),
    "tie_below": lambda: _planted(1100, 80, {(0, 0): 1.0, (70, 0): -9.0, (200, 0): 9.0, (1030, 0): 9.0}),
    "three_column_blocks": lambda: _dense(2 * _lu_constants()[1] + 1, 613),      # k_lu_update: three column blocks, the last one column (b) wide
}


@functools.lru_cache(maxsize=None)
def _large(name):
    """(A, b, np.linalg.solve, the model's swaps, the model's relative difference) of a LARGE system: about 2 s of NumPy hal::LU, once."""
    A, b = LARGE[name]()
    x, swaps = M.hal_lu_solve(A, b)
    want = np.linalg.solve(A, b)
    return A, b, want, swaps, float(np.max(np.abs(x - want) / np.abs(want)))


@pytest.mark.parametrize("name", sorted(LARGE))
def test_solver_alone_past_one_stride(gpu, name):
    """Systems larger than one stride of the pivot search (LU_PNT rows) and of k_lu_update's column block (LU_NT): the swaps are the model's,
    x by the rule of _systems() - 4 x the largest relative difference between np.linalg.solve and the NumPy hal::LU over the systems used
    (those of _systems() and this one), at most 1e-9."""
    from imagestitch_amd import exposure
    pnt, nt = _lu_constants()
    A, b, want, model_swaps, diff = _large(name)
    n = b.size
    rtol = min(4 * max(diff, _systems()[2] / 4), 1e-9)
    if name == "pivot_in_the_second_stride":
        assert n == pnt + 1 and int(np.argmax(np.abs(A[:, 0]))) == pnt and model_swaps >= 1
    elif name == "pivots_past_one_stride":
        assert n > pnt and int(np.argmax(np.abs(A[:, 0]))) == 1050 >= pnt and int(np.argmax(np.abs(A[:, 3]))) == n - 1 and model_swaps >= 2
    elif name == "tie_diagonal":
        tied = np.flatnonzero(np.abs(A[:, 0]) == np.abs(A[:, 0]).max())
        assert list(tied) == [0, 70, 1030] and tied[-1] >= pnt and int(np.argmax(np.abs(A[:, 0]))) == 0        # the model: no swap at column 0
    elif name == "tie_below":
        tied = np.flatnonzero(np.abs(A[:, 0]) == np.abs(A[:, 0]).max())
        assert list(tied) == [70, 200, 1030] and abs(A[0, 0]) < 9.0 and model_swaps >= _large("tie_diagonal")[3] + 1
    else:
        assert n == 2 * nt + 1 and -(-n // nt) == 3 and n - 2 * nt == 1                  # step 0 updates columns 1..n: LU_NT, LU_NT and column n alone
    x, swaps = exposure.lu_solve(A, b)
    print("%s: n %d, swaps %d (model %d), largest relative difference to np.linalg.solve %.3g (the model's %.3g, rtol %.3g)"
          % (name, n, swaps, model_swaps, np.max(np.abs(x - want) / np.abs(want)), diff, rtol))
    assert swaps == model_swaps
    np.testing.assert_allclose(x, want, rtol=rtol, atol=0)
    xh, _ = exposure.lu_solve(A, b, where="host")
    np.testing.assert_allclose(xh, want, rtol=rtol, atol=0)


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
    # a workgroup's footprint is 4 * 64 = 256 columns x 4 * 4 = 16 rows (asserted against BA_PX, BA_ROWS below): one less, exactly, one more
    "w255_h15": (255, 15, 32, 32), "w256_h16": (256, 16, 32, 32), "w257_h17": (257, 17, 32, 32),
    "w511_h16": (511, 16, 32, 32), "w512_h17": (512, 17, 32, 32), "w513_h15": (513, 15, 32, 32),
    # one row of less than, exactly and more than one group of four pixels
    "w1_h1": (1, 1, 32, 32), "w2_h1": (2, 1, 32, 32), "w3_h1": (3, 1, 32, 32), "w4_h1": (4, 1, 32, 32), "w5_h1": (5, 1, 32, 32),
    "map_1_wide_5_high": (20, 40, 32, 8),         # no tap to the right of any column: S[sx] alone
    "map_5_wide_1_high": (40, 20, 8, 32),         # both row indices clamp to row 0
}
EDGE_WIDTHS, EDGE_HEIGHTS = [4 * 64 * k + d for k in (1, 2) for d in (-1, 0, 1)], [15, 16, 17]


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
    img[0, 0] = (255, 90, 180)                                     # the bright corner: one byte saturates, two do not (an image of one pixel has no other)
    return comp, maps, img


APPLY_WHERE = ["host", "device", "host_odd", "device_odd", "device_aligned"]


def _apply_and_compare(comp, index, img, want, where, seed):
    """apply(index) on a copy of img as `where` says: exactly `want`; in a guard band, the image's bytes and nothing beside them."""
    if where == "host":
        a = img.copy()
        assert comp.apply(index, (0, 0), a) is a and np.array_equal(a, want)
    elif where == "device":
        t = _dev(img)
        comp.apply(index, (0, 0), t, None)
        assert np.array_equal(_np(t), want)
    else:
        place, layout = where.split("_")
        g = guarded.guarded_like(img, place, layout, seed)
        comp.apply(index, (0, 0), g.view)
        if place == "device":
            import torch
            torch.cuda.synchronize()
        g.check()
        assert np.array_equal(g.get(), want)


@pytest.mark.parametrize("where", APPLY_WHERE)
@pytest.mark.parametrize("name", sorted(APPLY))
def test_apply(gpu, name, where):
    """Bit for bit the model's apply on the library's own maps; in a guard band, the image's bytes and nothing beside them."""
    comp, maps, img = _fed(name)
    for index in (0, 1):
        want = M.apply_model(img, maps[index])
        if index == 0:
            assert np.any((img.astype(F32) * M.gain_image(maps[0], img.shape[1], img.shape[0])[:, :, None]) > 255.5)      # saturates at 255
            assert want.max() == 255 and not np.array_equal(want, img)
        _apply_and_compare(comp, index, img, want, where, 3 + index)


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


@pytest.mark.parametrize("where", APPLY_WHERE)
def test_apply_on_more_sizes(gpu, where):
    """Images of another size than the one fed, bit for bit the model's apply on the library's own maps.  A map LARGER than the image - in x
    only, in y only, in both, and larger in y but smaller in x - from one-pixel blocks on a 13 x 7 tile; every width around one and two
    workgroups' 256 columns with every height around a workgroup's 16 rows, under a 3 x 2 map; maps one block wide and one block high
    under sizes that cross a workgroup."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity
    c = fuzz_parity._kernel_consts("blocks_gain.hip")
    assert EDGE_WIDTHS == [c["BA_PX"] * 64 * k + d for k in (1, 2) for d in (-1, 0, 1)] and EDGE_HEIGHTS == [4 * c["BA_ROWS"] + d for d in (-1, 0, 1)]
    rng = np.random.default_rng(10)
    comp, maps, _ = _fed("map_of_the_images_size")
    mh, mw = maps[0].shape
    assert (mw, mh) == (13, 7)
    sizes = [(5, 7), (13, 3), (4, 3), (40, 3)]
    assert [(w < mw, h < mh) for w, h in sizes] == [(True, False), (False, True), (True, True), (False, True)] and sizes[3][0] > mw
    runs = [(comp, maps, 0, sizes)]
    comp, maps, _ = _fed("map_3x2")
    runs.append((comp, maps, 1, [(w, h) for w in EDGE_WIDTHS for h in EDGE_HEIGHTS]))
    for name in ("map_1_wide_5_high", "map_5_wide_1_high"):
        comp, maps, _ = _fed(name)
        assert maps[0].shape == ((5, 1) if name == "map_1_wide_5_high" else (1, 5))
        runs.append((comp, maps, 0, [(257, 17), (3, 50), (50, 3), (1, 1)]))
    for comp, maps, index, sizes in runs:
        for k, (w, h) in enumerate(sizes):
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            want = M.apply_model(img, maps[index])
            assert w * h < 64 or not np.array_equal(want, img)
            _apply_and_compare(comp, index, img, want, where, 70 + k)


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
    # a CUDAGraph that a dead reference cycle still holds (a test frame kept by its own pytest.raises info) must not be freed by a collection
    # that happens to run inside this capture: its destructor synchronises the device, which a capturing stream turns into an abort
    gc.collect()
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


def test_a_captured_apply_replays_under_a_later_feed_of_the_same_sizes(gpu):
    """The contract of isx_blocks_gain_apply: a graph captured before a later feed of images of the same sizes reads that feed's maps.
    What the captured launch keeps: the maps' device buffer plus the image's offset in it, the map's width, and the resize tables.  The
    buffer holds at most BG_MAX_BLOCKS = 16384 floats and DevBuf::reserve rounds every allocation up to 1 MiB, so it is allocated by the
    first feed and never again; the offset and width are those of the block grids, which equal sizes give again; the tables are kept
    until destroy.  (After a feed of OTHER sizes the captured offset and width are stale: outside the contract, not replayed here.)
    Also the copy path (one-pixel blocks, no tables at all)."""
    import torch
    for name, other, blocks in (("two_tiles", "dark_against_bright", (32, 32)), ("one_pixel_blocks", None, (1, 1))):
        corners, imgs, masks, _ = cases.case(name)
        imgs2 = cases.case(other)[1] if other else [(255 - a // 2).astype(np.uint8) for a in imgs]
        assert [a.shape for a in imgs2] == [a.shape for a in imgs] and not np.array_equal(imgs2[0], imgs[0])
        s = torch.cuda.Stream()
        comp = gpu.BlocksGainCompensator(*blocks, stream=s)
        with torch.cuda.stream(s):
            comp.feed(corners, imgs, masks)
            tile = _dev(imgs[0])
        torch.cuda.synchronize()
        maps1 = comp.gain_maps()
        g = torch.cuda.CUDAGraph()
        gc.collect()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            comp.apply(0, corners[0], tile)
        torch.cuda.synchronize()
        assert np.array_equal(_np(tile), imgs[0])                  # captured, not run
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(tile), M.apply_model(imgs[0], maps1[0]))
        with torch.cuda.stream(s):
            comp.feed(corners, imgs2, masks)                       # the same sizes and corners, other exposures
        torch.cuda.synchronize()
        maps2 = comp.gain_maps()
        assert maps2[0].shape == maps1[0].shape
        want1, want2 = M.apply_model(imgs[0], maps1[0]), M.apply_model(imgs[0], maps2[0])
        assert not np.array_equal(want1, want2)                    # the two feeds are told apart by the tile
        with torch.cuda.stream(s):
            tile.copy_(torch.from_numpy(imgs[0]))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(tile), want2), name


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
