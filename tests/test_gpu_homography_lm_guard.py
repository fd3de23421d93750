"""isx_find_homography_lm on mats inside guard bands (tests/helpers/guarded.py), host and device, aligned and unaligned: it writes H, the 12
stats columns, conf and the mask rows [0, count) and nothing else - not its inputs, not a mask row past the count, not a byte of pitch."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import homography_lm_cases as lmc  # noqa: E402
from helpers import guarded  # noqa: E402
from helpers import homography_lm_np as lm  # noqa: E402
from imagestitch_amd import homography as hg  # noqa: E402

pytestmark = pytest.mark.gpu
SPARE = 5          # rows of capacity past the count
NAMES = ["noise25_invert", "n5_below_thresh1", "collinear_40", "inliers_6"]
_WANT = []


def want():
    if not _WANT:
        named = lmc.named()
        _WANT.extend(lm.find_homography_lm_np(named[k][0], reproj_thresh=6.0, lm_max_iters=7) for k in NAMES)
    return _WANT


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("layout", guarded.LAYOUTS)
def test_only_the_outputs_are_written(gpu, where, layout):
    import torch
    named = lmc.named()
    sets = [named[k][0] for k in NAMES]
    assert all(w["margin"] >= 1e-9 for w in want()) and want()[0]["stats"][9] > 0
    g_p, g_m = [], []
    for i, p in enumerate(sets):
        full = np.random.default_rng(i).uniform(-9, 9, (len(p) + SPARE, 4)).astype(np.float32)
        full[:len(p)] = p
        g_p.append(guarded.guarded_like(full, where, layout, 10 + i, "points %d" % i))
        g_m.append(guarded.guarded((len(p) + SPARE, 1), np.uint8, where, layout, 20 + i, "mask %d" % i))
    g_c = guarded.guarded_like(np.array([[len(p) for p in sets]], np.int32), where, layout, 30, "counts")
    g_H = guarded.guarded((3 * len(sets), 3), np.float64, where, layout, 31, "H")
    g_s = guarded.guarded((len(sets), 12), np.int32, where, layout, 32, "stats")
    g_f = guarded.guarded((1, len(sets)), np.float64, where, layout, 33, "conf")
    info = hg.find_homography([g.view for g in g_p], g_c.view, g_H.view, [g.view for g in g_m], g_s.view, g_f.view, reproj_thresh=6.0, refine=True,
                              lm_max_iters=7)
    torch.cuda.synchronize()
    assert info == (len(sets), 1)
    g_c.check(written=guarded.NOTHING)
    for g in g_p:
        g.check(written=guarded.NOTHING)
    g_H.check()
    g_s.check()
    g_f.check()
    for k, w in enumerate(want()):
        n = 0 if w["mask"] is None else len(w["mask"])
        may = np.zeros(g_m[k].shape, bool)
        may[:n] = True
        g_m[k].check(written=may)
        assert np.array_equal(g_m[k].get()[:n, 0], w["mask"] if n else np.zeros(0, np.uint8)), NAMES[k]
        assert np.array_equal(g_s.get()[k], w["stats"]), NAMES[k]
        assert np.array_equal(np.ascontiguousarray(g_H.get()[3 * k:3 * k + 3]).view(np.uint64), w["H"].view(np.uint64)), NAMES[k]
        assert np.float64(g_f.get()[0, k]).view(np.uint64) == np.float64(w["conf"]).view(np.uint64), NAMES[k]
