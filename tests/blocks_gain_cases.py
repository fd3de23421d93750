"""The tile sets tests/test_blocks_gain_model.py (CPU) and tests/test_gpu_blocks_gain.py (GPU) share, and their models, computed once."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import blocks_gain_np as M  # noqa: E402

CORNERS2 = [(0, 0), (37, 5)]          # tile 0 is 100 x 80 (4 x 3 blocks of 25 x 27), tile 1 is 90 x 70 (3 x 3 blocks of 30 x 24): 21 blocks, and
SIZES2 = [(100, 80), (90, 70)]        # every block of one meets up to four of the other


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


@functools.lru_cache(maxsize=None)
def case(name):
    """(corners, images, masks, model) - computed once per process; treat as read-only."""
    corners, imgs, masks = CASES[name]()
    return corners, imgs, masks, M.feed_blocks_model(corners, imgs, masks)


def lu_rel_diff(name):
    """The largest relative difference between np.linalg.solve and the NumPy hal::LU on a case's system, and hal::LU's row swaps."""
    _, _, _, model = case(name)
    x, swaps = M.hal_lu_solve(model["A"], model["b"])
    return float(np.max(np.abs(x - model["gains"]) / np.abs(model["gains"]))), swaps
