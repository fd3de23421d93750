"""Where detectResultRoi's four extrema sit on the scan rigs of tests/polar_cases.py, by the NumPy model alone (no GPU): k_polar_roi_scan
reduces 256 columns x 16 rows a block through shuffles (64 lanes), LDS (4 waves) and four atomics (the blocks), and the case set must put an
extremum into every position that reduction distinguishes.  A condition on the cases, not on the library: a rig that stops reaching the class
it is listed for fails here, and tests/test_gpu_polar_scan.py then compares the device's answer on exactly these rigs with the model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
from helpers import polar_np as P  # noqa: E402

KINDS = [P.FISHEYE, P.STEREOGRAPHIC]


def census(name, kind):
    w, h, f, K, R = PC.scan_rig(name, kind)
    where = PC.scan_extrema(P.from_rig(kind, f, K, R), w, h)
    assert all(p is not None for p in where), (name, kind, where)
    got = set()
    for x, y in where:
        got |= PC.scan_classes(x, y, w, h)
    return got, where


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(PC.SCAN_RIGS))
def test_each_scan_rig_reaches_the_classes_it_is_listed_for(name, kind):
    got, where = census(name, kind)
    print(name, PC.KIND_NAMES[kind], where, sorted(got))
    missing = set(PC.SCAN_RIGS[name][6]) - got
    assert not missing, (name, kind, where, sorted(missing))


@pytest.mark.parametrize("kind", KINDS)
def test_the_scan_rigs_reach_every_class(kind):
    listed, reached = set(), set()
    for name in PC.SCAN_RIGS:
        listed |= set(PC.SCAN_RIGS[name][6])
        reached |= census(name, kind)[0]
    assert listed == set(PC.SCAN_CLASSES), sorted(set(PC.SCAN_CLASSES) - listed)        # (and each listed one is reached: the test above)
    assert reached >= set(PC.SCAN_CLASSES)
    sizes = {PC.SCAN_RIGS[n][:2] for n in PC.SCAN_RIGS}
    assert sizes >= {(1, 1), (1, 40), (300, 1), (256, 16), (257, 17)} and max(s[0] for s in sizes) == 800


def test_the_classes_of_a_pixel():
    """scan_classes itself, on hand-computed positions of a 600 x 37 source (column blocks 0-255, 256-511, 512-599; row bands 0-15, 16-31, 32-36)."""
    assert PC.scan_classes(0, 0, 600, 37) == {"col_block_0"}
    assert PC.scan_classes(40, 20, 600, 37) == {"col_block_0", "lane_32plus", "middle_full_row_band", "interior"}
    assert PC.scan_classes(256, 36, 600, 37) == {"col_block_1", "wave_0", "partial_last_row_band"}
    assert PC.scan_classes(511, 1, 600, 37) == {"col_block_1", "wave_3", "lane_32plus", "interior"}
    assert PC.scan_classes(599, 31, 600, 37) == {"col_block_2plus", "wave_1", "partial_last_col_block", "middle_full_row_band"}
    assert PC.scan_classes(255, 15, 256, 16) == {"col_block_0", "lane_32plus"}          # full blocks: nothing partial
    assert PC.scan_classes(0, 0, 1, 1) == {"col_block_0", "partial_last_col_block", "partial_last_row_band"}


def test_the_nan_camera_in_the_model():
    """mapForward is NaN on every pixel of the degenerate camera: min / max keep +-FLT_MAX, the four casts give INT_MIN."""
    K, R = PC.NAN_CAMERA
    for kind in KINDS:
        m = P.from_rig(kind, 25.0, K, R)
        assert np.isfinite(m.r_kinv).all() and np.isfinite(m.k_rinv).all()
        xs, ys = np.meshgrid(np.arange(8).astype(np.float32), np.arange(6).astype(np.float32))
        u, v = m.map_forward(xs, ys)
        assert np.isnan(u).all() and np.isnan(v).all()
        roi, mm = m.detect_roi(8, 6)
        fmax = np.finfo(np.float32).max
        assert list(roi) == [P.INT_MIN] * 4 and np.array_equal(mm, np.array([fmax, fmax, -fmax, -fmax], np.float32))
        assert PC.scan_extrema(m, 8, 6) == [None] * 4
