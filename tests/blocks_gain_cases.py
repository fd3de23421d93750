"""The tile sets tests/test_blocks_gain_model.py (CPU) and tests/test_gpu_blocks_gain.py (GPU) share, and their models, computed once.

CASES are the four sets of 32 x 32 blocks whose records are one work item each.  MORE are the sets that reach where those do not: three tiles
that all meet, records of several work items, a row wider than an item, no off-diagonal record at all, one-pixel blocks; each with its own
block size.  What a set
of MORE is for is computed from its geometry and gain.hip's constants (record_items), never taken on trust: a set that stops reaching its
path fails its test."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_parity as F  # noqa: E402
from helpers import blocks_gain_np as M  # noqa: E402

# the band formula, the records of a tile set and the forward-error rtol live with the fuzz family that draws its cases by them
bands, record_items, forward_error_rtol = F.bg_bands, F.bg_record_items, F.bg_forward_error_rtol

CORNERS2 = [(0, 0), (37, 5)]          # tile 0 is 100 x 80 (4 x 3 blocks of 25 x 27), tile 1 is 90 x 70 (3 x 3 blocks of 30 x 24): 21 blocks, and
SIZES2 = [(100, 80), (90, 70)]        # every block of one meets up to four of the other
MASK_VALUES = np.array([0, 254, 255, 255, 255, 255], np.uint8)


def _tile(w, h, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, 3), dtype=np.uint8)


def _full(w, h):
    return np.full((h, w), 255, np.uint8)


def two_tiles():
    imgs = [_tile(w, h, 40 + k, 30 * k, 200 + 50 * k) for k, (w, h) in enumerate(SIZES2)]
    return CORNERS2, imgs, [_full(w, h) for w, h in SIZES2]


def two_tiles_holes():
    """Tile 0's mask has a hole (with 254s on its rim: they do not count), tile 1's a zero band over its first 13 columns - global columns 37..49,
    all that tile 0's block column 1 (25..49) shares with tile 1's block column 0 (37..66): five pairs of blocks meet in no counted pixel."""
    corners, imgs, masks = two_tiles()
    masks = [m.copy() for m in masks]
    masks[0][20:47, 60:81] = 0
    masks[0][19, 60:81] = 254
    masks[1][:, :13] = 0
    return corners, imgs, masks


def dark_against_bright():
    """Tile 0 bytes in [10, 60), tile 1 in [200, 256): the system's off-diagonal entries outweigh some diagonal ones and hal::LU swaps rows."""
    imgs = [_tile(100, 80, 51, 10, 60), _tile(90, 70, 52, 200, 256)]
    return CORNERS2, imgs, [_full(w, h) for w, h in SIZES2]


def three_tiles():
    """Tiles 0 and 2 are apart; tile 1 meets both."""
    sizes = [(70, 50), (80, 45), (60, 66)]
    corners = [(0, 0), (50, 10), (115, -8)]
    rng = np.random.default_rng(7)
    imgs = [_tile(w, h, 60 + k, 10 * k, 180 + 30 * k) for k, (w, h) in enumerate(sizes)]
    masks = [rng.choice(np.array([0, 254, 255, 255, 255, 255, 255], np.uint8), size=(h, w)) for w, h in sizes]
    return corners, imgs, masks


CASES = {"two_tiles": two_tiles, "two_tiles_holes": two_tiles_holes, "dark_against_bright": dark_against_bright, "three_tiles": three_tiles}


def _drawn(corners, sizes, seed):
    """Tiles of random bytes under masks drawn from {0, 254, 255 x 4}."""
    rng = np.random.default_rng(seed)
    imgs = [_tile(w, h, seed + 1 + k) for k, (w, h) in enumerate(sizes)]
    return corners, imgs, [rng.choice(MASK_VALUES, size=(h, w)) for w, h in sizes]


def several_items():
    """2 x 1 blocks of 150 x 200 and of 140 x 190 pixels: every block is two diagonal work items, the second shorter, and the pairs of blocks
    that meet share more pixels than one off-diagonal item holds, in a height that is no multiple of the band."""
    return _drawn([(0, 0), (37, 5)], [(300, 200), (280, 190)], 300)


def row_wider_than_an_item():
    """One block per tile; the blocks meet in 2 rows of 4097 pixels: the band is one row, longer than an off-diagonal item's nominal size."""
    return _drawn([(0, 0), (-3, 1)], [(4100, 3), (4100, 4)], 310)


def mask_row_wider_than_an_item():
    """One block per tile; tile 0's is 2 rows of 16400 mask bytes: the band is one row, longer than a diagonal item's nominal size."""
    return _drawn([(0, 0), (100, 1)], [(16400, 2), (600, 2)], 320)


def one_image():
    return _drawn([(5, 5)], [(40, 30)], 330)


def apart():
    return _drawn([(0, 0), (100, 100)], [(40, 30), (20, 20)], 340)


def one_pixel_blocks():
    """Every pixel a block: 63 + 48 = 111 unknowns, maps of the images' sizes (apply takes the copy path).  A dark tile against a bright one, full
    masks: off-diagonal entries outweigh diagonal ones and hal::LU swaps rows."""
    sizes = [(9, 7), (8, 6)]
    imgs = [_tile(9, 7, 351, 10, 60), _tile(8, 6, 352, 200, 256)]
    return [(0, 0), (4, 3)], imgs, [_full(w, h) for w, h in sizes]


def three_tiles_all_meet():
    """Every tile meets both others: the records by (block_i, block_j) are not the records image pair by image pair - tile 0's blocks against
    tile 2's come before tile 0's later blocks against tile 1's."""
    return _drawn([(0, 0), (50, 10), (40, -8)], [(70, 50), (80, 45), (60, 66)], 360)


MORE = {"three_tiles_all_meet": (three_tiles_all_meet, (32, 32)), "several_items": (several_items, (200, 200)), "row_wider_than_an_item": (row_wider_than_an_item, (8192, 32)),
        "mask_row_wider_than_an_item": (mask_row_wider_than_an_item, (16400, 32)), "one_image": (one_image, (8, 8)), "apart": (apart, (32, 32)),
        "one_pixel_blocks": (one_pixel_blocks, (1, 1))}
NO_PAIRS = ("one_image", "apart")


def blocks(name):
    """(bl_width, bl_height) of a set."""
    return MORE[name][1] if name in MORE else (32, 32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(corners, images, masks, model) - computed once per process; treat as read-only."""
    corners, imgs, masks = (CASES[name] if name in CASES else MORE[name][0])()
    return corners, imgs, masks, M.feed_blocks_model(corners, imgs, masks, *blocks(name))


def lu_rel_diff(name):
    """The largest relative difference between np.linalg.solve and the NumPy hal::LU on a case's system, and hal::LU's row swaps."""
    _, _, _, model = case(name)
    x, swaps = M.hal_lu_solve(model["A"], model["b"])
    return float(np.max(np.abs(x - model["gains"]) / np.abs(model["gains"]))), swaps


@functools.lru_cache(maxsize=None)
def gain_rtol(name):
    """forward_error_rtol of a set's model: (rtol, the measured CPU difference)."""
    _, _, _, model = case(name)
    return forward_error_rtol(model["A"], model["b"], model["gains"])


# ---- what the library's work table looks like for a set, from the geometry ---------------------------------------------------------------------

def kernel_constants():
    """GF_DIAG_BYTES and GF_PAIR_PIXELS as gain.hip defines them (read from the source by tools/fuzz_parity.py's reader)."""
    return F._GF["GF_DIAG_BYTES"], F._GF["GF_PAIR_PIXELS"]


def items_of(name):
    corners, imgs, _, _ = case(name)
    return record_items(corners, [(a.shape[1], a.shape[0]) for a in imgs], *blocks(name), *kernel_constants())


def premise(name):
    """What a set of MORE is there for, computed from its geometry, the model and gain.hip's constants."""
    _, imgs, _, model = case(name)
    diag_bytes, pair_pixels = kernel_constants()
    diag, pairs = items_of(name)
    assert len(diag) == len(model["diag_n"]) and len(pairs) == len(model["pairs"])
    print("%s: bands of the blocks %s, of the pairs %s" % (name, [b for _, _, b in diag][:6], [b for _, _, b in pairs][:6]))
    if name == "three_tiles_all_meet":
        by_image_pair = sorted(model["pairs"], key=lambda p: (model["owner"][p[0]], model["owner"][p[1]], p[0], p[1]))
        assert {(model["owner"][p[0]], model["owner"][p[1]]) for p in model["pairs"]} == {(0, 1), (0, 2), (1, 2)} and by_image_pair != model["pairs"]
    elif name == "several_items":
        assert model["counts"] == [(2, 1), (2, 1)] and (diag[0][0], diag[0][1]) == (150, 200)
        assert any(len(b) >= 2 for _, _, b in diag) and any(len(b) >= 2 for _, _, b in pairs)
        assert any(len(b) >= 2 and b[-1] < b[0] for _, _, b in diag + pairs)
        assert all(len(b) == 2 and 0 < b[1] < b[0] for _, _, b in diag)                   # every block: two items, the second shorter
        assert any(w * h > pair_pixels and h % b[0] for w, h, b in pairs)
    elif name == "row_wider_than_an_item":
        assert model["counts"] == [(1, 1), (1, 1)] and pairs == [(pair_pixels + 1, 2, [1, 1])]
    elif name == "mask_row_wider_than_an_item":
        assert model["counts"] == [(1, 1), (1, 1)] and diag[0] == (16400, 2, [1, 1]) and diag[0][0] > diag_bytes
    elif name in NO_PAIRS:
        assert pairs == [] and model["pairs"] == []
        assert np.all(model["gains"] == 1.0) and all(np.all(m == np.float32(1)) for m in model["maps"])        # diag and b are the same sums
    elif name == "one_pixel_blocks":
        swaps = lu_rel_diff(name)[1]
        print("%s: the model's hal::LU swaps rows %d times" % (name, swaps))
        assert len(diag) == 111 and swaps > 0
        assert [m.shape for m in model["maps"]] == [a.shape[:2] for a in imgs]           # apply takes the copy path
