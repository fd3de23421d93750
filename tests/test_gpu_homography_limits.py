"""isx_find_homography and isx_find_homography_lm past the counts of their first suites, bit-exact against tests/helpers/homography_np.py and
homography_lm_np.py under the rules of test_gpu_homography.check (stats and masks with np.array_equal, H and conf through their uint64
views, sentinels past the count untouched):
  correspondences per pair   127 / 128 / 129 (either side of two ballots), 2 000, 8 193 and a half-outlier 4 096: the ballot-per-64 scoring
                             loop, the in-order compaction into the scratch, pass 2 on thousands of inliers, the refit whose lanes walk every
                             inlier, the LM polish's walks; host, strided and guarded layouts, counts past and below the rows at 8 193
  the confidence boundary    240 exact correspondences give 240 / 80 = 3, 241 give more and so 0
  pairs per call             2 016 point sets (a 64-image rig's pairs) in one launch of one block a pair at occupancy 1, the per-pair scratch
                             carved out of one buffer: each pair equals its model and the same set run alone
tests/test_homography_model.py holds on the CPU what the cases are (homography_cases.limits, mixed_2016)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import homography_cases as cases  # noqa: E402
import test_gpu_homography as TH  # noqa: E402  (its run_raw and check)
import test_gpu_homography_lm as TL  # noqa: E402  (the same for the entry with the polish)
from helpers import guarded  # noqa: E402
from helpers import homography_lm_np as lm  # noqa: E402
from helpers import homography_np as hm  # noqa: E402
from imagestitch_amd import homography as hg  # noqa: E402

pytestmark = pytest.mark.gpu
LIMITS = cases.limits()
THOUSANDS = ["n2000_noisy", "n8193_noisy"]
SENT_F, SENT_B = TH.SENT_F, TH.SENT_B


@functools.lru_cache(maxsize=None)
def model(name, count=None):
    w = hm.find_homography_np(LIMITS[name], count=count)
    assert w["margin"] >= 1e-6
    return w


@functools.lru_cache(maxsize=None)
def model_lm(name, iters):
    w = lm.find_homography_lm_np(LIMITS[name], lm_max_iters=iters)
    assert w["margin"] >= 1e-6
    return w


@pytest.mark.parametrize("name", sorted(LIMITS))
def test_limit_cases_on_device_mats(gpu, name):
    """0.01 - 0.25 s each; the model of the 8 193 set takes 0.45 s of CPU."""
    got, info = TH.run_raw([LIMITS[name]])
    TH.check(got[0], model(name), name)
    assert info == (1, 1)


def test_the_confidence_boundary(gpu):
    got, _ = TH.run_raw([LIMITS["n240_exact"], LIMITS["n241_exact"]])
    assert [g["conf"] for g in got] == [3.0, 0.0] and [int(g["stats"][hg.NUM_INLIERS]) for g in got] == [240, 241]
    assert all(g["stats"][hg.STATUS] == hg.ST_H | hg.ST_PASS2 for g in got)      # conf 0 with a homography and all its inliers


@pytest.mark.parametrize("name", THOUSANDS)
def test_thousands_on_host_mats_and_in_wide_layouts(gpu, name):
    pts = LIMITS[name]
    got, info = TH.run_raw([pts], device=False)
    TH.check(got[0], model(name), (name, "host"))
    assert info == (1, 1)
    for device in (True, False):
        got, _ = TH.run_raw([pts], device=device, extra_rows=7, wide=True)
        TH.check(got[0], model(name), (name, device, "wide"))
        assert np.array_equal(got[0]["points"][:len(pts), :4], pts) and (got[0]["points"][len(pts):] == np.float32(SENT_F)).all()


def test_counts_past_and_below_the_rows_at_8193(gpu):
    name = "n8193_noisy"
    pts = LIMITS[name]
    want = model(name, 8194)                                          # one past the rows: clamped, status bit 3
    assert want["stats"][0] == model(name)["stats"][0] | hg.ST_CLAMPED and np.array_equal(want["stats"][1:], model(name)["stats"][1:])
    got, _ = TH.run_raw([pts], counts=[8194])
    TH.check(got[0], want, "clamped")
    want = model(name, 2000)                                          # the rest is capacity: mask rows 2 000 .. 8 192 keep their sentinels
    assert len(want["mask"]) == 2000 and want["stats"][0] == hg.ST_H | hg.ST_PASS2
    got, _ = TH.run_raw([pts], counts=[2000])
    TH.check(got[0], want, "2000 of 8193")
    assert (got[0]["mask"][2000:] == SENT_B).all()


@pytest.mark.parametrize("iters", [10, 1])
@pytest.mark.parametrize("name", THOUSANDS)
def test_the_lm_polish_on_thousands(gpu, name, iters):
    """The model with the polish takes 0.9 s at 8 193 correspondences and 10 iterations."""
    want = model_lm(name, iters)
    assert want["stats"][hg.LM_NFJ1] > 0 and want["stats"][hg.LM_NFJ2] > 0 and (want["stats"][hg.LM_RET1] == -1) == (iters == 1)
    got, info = TL.run_raw([LIMITS[name]], lm_max_iters=iters)
    TL.check(got[0], want, (name, iters))
    assert info == (1, 1)
    assert np.array_equal(got[0]["stats"][:7], model(name)["stats"][:7]) and np.array_equal(got[0]["mask"], model(name)["mask"])


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("layout", guarded.LAYOUTS)
def test_only_the_outputs_are_written_at_8193(gpu, where, layout):
    """The pattern of test_gpu_homography_guard.py with inlier buffers of 33 K floats a pair: nothing past `count` rows of the mask, and
    nothing outside H, stats and conf, is written."""
    import torch
    spare = 5
    pts, want = LIMITS["n8193_noisy"], model("n8193_noisy")
    full = np.random.default_rng(1).uniform(-9, 9, (len(pts) + spare, 4)).astype(np.float32)
    full[:len(pts)] = pts
    g_p = guarded.guarded_like(full, where, layout, 10, "points")
    g_m = guarded.guarded((len(pts) + spare, 1), np.uint8, where, layout, 20, "mask")
    g_c = guarded.guarded_like(np.array([[len(pts)]], np.int32), where, layout, 30, "counts")
    g_H = guarded.guarded((3, 3), np.float64, where, layout, 31, "H")
    g_s = guarded.guarded((1, 8), np.int32, where, layout, 32, "stats")
    g_f = guarded.guarded((1, 1), np.float64, where, layout, 33, "conf")
    info = hg.find_homography([g_p.view], g_c.view, g_H.view, [g_m.view], g_s.view, g_f.view)
    torch.cuda.synchronize()
    assert info == (1, 1)
    g_c.check(written=guarded.NOTHING)
    g_p.check(written=guarded.NOTHING)
    g_H.check()
    g_s.check()
    g_f.check()
    may = np.zeros(g_m.shape, bool)
    may[:len(pts)] = True
    g_m.check(written=may)
    assert np.array_equal(g_m.get()[:len(pts), 0], want["mask"]) and np.array_equal(g_s.get()[0], want["stats"])
    assert np.array_equal(np.ascontiguousarray(g_H.get()).view(np.uint64), want["H"].view(np.uint64))
    assert np.float64(g_f.get()[0, 0]).view(np.uint64) == np.float64(want["conf"]).view(np.uint64)


def _mixed(run_raw, check, find, **more):
    sets, names, kw = cases.mixed_2016()
    kw = dict(kw, **more)
    want = {n: find(p, **kw) for n, p in sets.items()}
    assert min(w["margin"] for w in want.values()) >= 1e-9
    got, info = run_raw([sets[n] for n in names], **kw)
    assert info == (2016, 1)
    for k, n in enumerate(names):
        check(got[k], want[n], (k, n))
    for n, p in sets.items():                                         # each distinct set alone: the bytes of every place it stands at
        alone, _ = run_raw([p], **kw)
        for k in (k for k, m in enumerate(names) if m == n):
            assert all(np.array_equal(alone[0][key], got[k][key]) for key in ("H", "mask", "stats")), (k, n)
            assert np.float64(alone[0]["conf"]).view(np.uint64) == np.float64(got[k]["conf"]).view(np.uint64), (k, n)


def test_2016_pairs_in_one_call(gpu):
    """The models of the 42 distinct sets take 5.5 s of CPU (outliers_to_the_end at max_iters = 2 000 alone 1.2 s), the test 3.3 s on an MI355X box."""
    _mixed(TH.run_raw, TH.check, hm.find_homography_np)


def test_2016_pairs_in_one_call_with_the_lm_polish(gpu):
    """The same call through isx_find_homography_lm, lm_max_iters = 10, 12 stats columns: the models take 6.0 s of CPU (3.5 s the test on an
    MI355X box), so the substantive sets are not halved."""
    _mixed(TL.run_raw, TL.check, lm.find_homography_lm_np, lm_max_iters=10)
