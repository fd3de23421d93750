"""tests/helpers/estimator_np.py - the specification of isx_estimate_cameras - against facts that do not come from the model: planted
focals and rotations, hand-computed focals for every branch of C:40-43 and C:50-53, the medians, the fallback, trees whose centers are
known, the tie rule, the named cases of tests/estimator_cases.py being what their names say, and the fuzz generator.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import estimator_cases as cases  # noqa: E402
from helpers import estimator_np as em  # noqa: E402

F = np.float64


def _run(c):
    return em.estimate_rig(c["sizes"], c["pairs"], c["H"], c["stats"], c["focals_in"])


def _tree_case(n, edges, weights=None):
    """A rig whose graph has exactly `edges` (planted homographies), weights given or all 100."""
    return cases.make(n, sorted(tuple(sorted(e)) for e in edges), 21, weights=100 if weights is None else weights)


@pytest.mark.parametrize("seed", range(12))
def test_planted_focal_and_rotations_come_back(seed):
    """H_ij = K R_j^T R_i K^-1 / h22: the focal within 1e-9 relative, the rotations relative to the root within 1e-9.  A homography has no
    scale, and C:236 takes H as it is: dividing by h22 multiplies every edge's R by that h22, so what comes back is s R with s the product of
    the h22 along the path (the reference leaves the scale to its bundle adjuster).  det(s R) = s^3 gives s; R itself is held to 1e-9."""
    n = 3 + seed % 5
    c = cases.make(n, cases.all_pairs(n), 100 + seed, focal=400.0 + 150.0 * seed)
    out = _run(c)
    rs = out["rig_stats"]
    assert rs[em.RIG_STATUS] == em.EST_MEDIAN and rs[em.RIG_CANDIDATES] == n * (n - 1) and rs[em.RIG_REACHED] == n
    assert np.all(np.abs(out["cameras"][:, 0] / c["focal"] - 1.0) <= 1e-9), out["cameras"][:, 0]
    root = int(np.where(out["tree"][:, 0] == -1)[0][0])
    for i in range(n):
        want = c["rotations"][root].T @ c["rotations"][i]
        got = out["cameras"][i, 4:13].reshape(3, 3)
        assert np.abs(got / np.cbrt(np.linalg.det(got)) - want).max() <= 1e-9, (i, root)
    assert np.array_equal(out["cameras"][:, 2:4], 0.5 * np.array(c["sizes"], np.float64)) and np.all(out["cameras"][:, 13:16] == 0)
    k32 = out["kr32"][:, :9].reshape(n, 3, 3)
    assert np.array_equal(k32[:, 0, 0], out["cameras"][:, 0].astype(np.float32)) and np.array_equal(k32[:, 0, 2], out["cameras"][:, 2].astype(np.float32))
    assert np.array_equal(out["kr32"][:, 9:], out["cameras"][:, 4:13].astype(np.float32))


def test_inv3_and_mul3_against_numpy():
    rng = np.random.default_rng(5)
    for _ in range(50):
        a, b = rng.uniform(-2, 2, (3, 3)), rng.uniform(-2, 2, (3, 3))
        assert np.allclose(np.array(em.inv3([F(v) for v in a.ravel()])).reshape(3, 3), np.linalg.inv(a), rtol=1e-9, atol=1e-12)
        assert np.allclose(np.array(em.mul3([F(v) for v in a.ravel()], [F(v) for v in b.ravel()])).reshape(3, 3), a @ b, rtol=1e-12, atol=1e-14)
    assert em.inv3([F(v) for v in (1, 2, 3, 2, 4, 6, 0, 1, 1)]) == [0.0] * 9          # a determinant of exactly 0: nine zeros


def _h(h0=1.0, h1=0.0, h2=0.0, h3=0.0, h4=1.0, h5=0.0, h6=0.0, h7=0.0):
    return [F(v) for v in (h0, h1, h2, h3, h4, h5, h6, h7, 1.0)]


def test_focals_from_homography_branches():
    with np.errstate(all="ignore"):
        # a pure yaw: h6 * h7 = 0 and h0 h1 + h3 h4 = 0 -> v1 = -0 / 0 = NaN falls through every comparison: not ok; f0 likewise (d1 = 0, h2 h5 = 0)
        H = cases.homography(cases.rotation(0, 0, 0), cases.rotation(0.2, 0, 0), 700.0)
        f0, f1, ok0, ok1 = em.focals_from_homography([F(v) for v in H.ravel()])
        assert not ok0 and not ok1
        # f1, C:41 both positive, |d1| > |d2| takes the larger (after the swap v1): h6 = 1, h7 = 2: d1 = 2, d2 = 3 -> |d1| < |d2| -> v2
        # v1 = -(h0 h1 + h3 h4) / 2, v2 = (h0^2 + h3^2 - h1^2 - h4^2) / 3
        h = _h(h0=3.0, h1=-1.0, h3=1.0, h4=-1.0, h6=1.0, h7=2.0)      # v1 = 4 / 2 = 2, v2 = (9 + 1 - 1 - 1) / 3 = 8/3 -> swap: v1 = 8/3, v2 = 2
        _, f1, _, ok1 = em.focals_from_homography(h)
        assert ok1 and f1 == np.sqrt(F(2.0))                          # |d1| = 2 < |d2| = 3: v2 (the smaller after the swap)
        h = _h(h0=3.0, h1=-1.0, h3=1.0, h4=-1.0, h6=3.0, h7=-2.0)     # d1 = -6, d2 = (-5)(1) = -5: v1 = 4 / -6 < 0, v2 = 8 / -5 < 0: not ok (C:43)
        assert not em.focals_from_homography(h)[3]
        h = _h(h0=3.0, h1=-1.0, h3=1.0, h4=-1.0, h6=2.0, h7=1.5)      # d1 = 3, d2 = -0.5 * 3.5 = -1.75: v1 = 4 / 3, v2 = 8 / -1.75 < 0: C:42
        _, f1, _, ok1 = em.focals_from_homography(h)
        assert ok1 and f1 == np.sqrt(F(4.0) / F(3.0))
        h = _h(h0=3.0, h1=-1.0, h3=1.0, h4=-1.0, h6=4.0, h7=5.0)      # d1 = 20, d2 = 9: both positive (0.2, 8/9), |d1| > |d2|: v1 = 8/9 after the swap
        _, f1, _, ok1 = em.focals_from_homography(h)
        assert ok1 and f1 == np.sqrt(F(8.0) / F(9.0))
        # f0: d1 = h0 h3 + h1 h4, d2 = h0^2 + h1^2 - h3^2 - h4^2, v1 = -h2 h5 / d1, v2 = (h5^2 - h2^2) / d2
        h = _h(h0=2.0, h1=0.0, h2=-3.0, h3=1.0, h4=1.0, h5=4.0)       # d1 = 2, d2 = 4 - 2 = 2: v1 = 12 / 2 = 6, v2 = 7 / 2: |d1| > |d2| false: v2
        f0, _, ok0, _ = em.focals_from_homography(h)
        assert ok0 and f0 == np.sqrt(F(3.5))
        h = _h(h0=3.0, h1=0.0, h2=-3.0, h3=1.0, h4=1.0, h5=4.0)       # d1 = 3, d2 = 7: v1 = 4, v2 = 1: |d1| < |d2|: v2 = 1
        assert em.focals_from_homography(h)[0] == 1.0
        h = _h(h0=1.0, h1=3.0, h2=-3.0, h3=1.0, h4=1.0, h5=4.0)       # d1 = 4, d2 = 8: v1 = 3, v2 = 7/8: v2
        assert em.focals_from_homography(h)[0] == np.sqrt(F(7.0) / F(8.0))
        h = _h(h0=1.0, h1=1.0, h2=-3.0, h3=3.0, h4=1.0, h5=4.0)       # d1 = 4, d2 = -8: v1 = 3, v2 = 7 / -8 < 0: C:52
        f0, _, ok0, _ = em.focals_from_homography(h)
        assert ok0 and f0 == np.sqrt(F(3.0))
        h = _h(h0=1.0, h1=1.0, h2=3.0, h3=3.0, h4=1.0, h5=4.0)        # v1 = -12 / 4 < 0, v2 < 0: C:53
        assert not em.focals_from_homography(h)[2]


def _entries_with_focals(n, focals):
    """Ordered-pair entries whose candidates are exactly `focals`: H = diag-like matrices are hard to aim, so the median is checked on
    estimate_focal's own list through a stub of focals_from_homography."""
    return {(0, k + 1): ([F(f)] * 9, 1) for k, f in enumerate(focals)}


def test_medians_and_fallback(monkeypatch):
    monkeypatch.setattr(em, "focals_from_homography", lambda h: (h[0], h[0], True, True))     # the candidate is sqrt(f * f)
    sizes = [(100, 50)] * 6
    f, med, cnt = em.estimate_focal(6, sizes, _entries_with_focals(6, [9.0, 1.0, 4.0, 16.0, 25.0]))
    assert (f, med, cnt) == (9.0, True, 5)                                                    # odd: the middle one
    n = 5
    f, med, cnt = em.estimate_focal(n, sizes[:n], _entries_with_focals(n, [9.0, 1.0, 4.0, 16.0]))
    assert (f, med, cnt) == ((F(4.0) + F(9.0)) * F(0.5), True, 4)                             # even: the mean of the middle two, times 0.5
    f, med, cnt = em.estimate_focal(6, sizes, _entries_with_focals(6, [9.0, 1.0, 4.0, 16.0]))
    assert (f, med, cnt) == (150.0, False, 4)                                                 # count == num_images - 2: sum(w + h) / n
    f, med, cnt = em.estimate_focal(3, [(640, 480), (641, 480), (640, 481)], {})
    assert (f, med, cnt) == (F(3362.0) / F(3.0), False, 0)


def test_the_fallback_case_and_the_pure_yaw():
    out = _run(cases.named()["fallback_focal"])
    rs = out["rig_stats"]
    c = cases.named()["fallback_focal"]
    assert rs[em.RIG_STATUS] == 0 and rs[em.RIG_CANDIDATES] == 0 and rs[em.RIG_REACHED] == 5
    assert out["cameras"][0, 0] == sum(w + h for w, h in c["sizes"]) / 5.0


def test_tree_centers():
    out = _run(_tree_case(5, [(0, 1), (1, 2), (2, 3), (3, 4)]))                               # a path of 5: one center
    rs = out["rig_stats"]
    assert (rs[em.RIG_CENTER0], rs[em.RIG_CENTER1], rs[em.RIG_NUM_CENTERS], rs[em.RIG_MIN_MAX_DIST], rs[em.RIG_TREE_EDGES]) == (2, -1, 1, 2, 4)
    assert out["tree"][:, 0].tolist() == [1, 2, -1, 2, 3] and out["tree"][:, 1].tolist() == [2, 1, 0, 1, 2]
    out = _run(_tree_case(4, [(0, 1), (1, 2), (2, 3)]))                                       # a path of 4: two centers, the lower is the root
    rs = out["rig_stats"]
    assert (rs[em.RIG_CENTER0], rs[em.RIG_CENTER1], rs[em.RIG_NUM_CENTERS], rs[em.RIG_MIN_MAX_DIST]) == (1, 2, 2, 2)
    assert out["tree"][:, 0].tolist() == [1, -1, 1, 2]
    out = _run(_tree_case(6, [(3, k) for k in range(6) if k != 3]))                           # a star
    rs = out["rig_stats"]
    assert (rs[em.RIG_CENTER0], rs[em.RIG_NUM_CENTERS], rs[em.RIG_MIN_MAX_DIST]) == (3, 1, 1) and out["tree"][:, 0].tolist() == [3, 3, 3, -1, 3, 3]
    out = _run(cases.named()["demo_2_images_1_pair"])                                         # the demo's shape
    assert out["rig_stats"].tolist() == [em.EST_MEDIAN, 2, 0, 1, 1, 2, 2, 1] and out["tree"].tolist() == [[-1, 0], [0, 1]]


def test_the_maximum_spanning_tree_takes_the_heavy_edges():
    pairs = cases.all_pairs(4)                         # (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    out = _run(cases.make(4, pairs, 30, weights=[10, 90, 20, 30, 80, 70]))
    assert out["tree_edges"] == [(0, 2), (1, 3), (2, 3)]


def test_the_tie_rule_decides_when_all_weights_are_equal():
    """weight descending, then i * n + j ascending: with equal weights Kruskal takes (0, 1), (0, 2), ... (0, n - 1) - a star around 0."""
    c = cases.named()["all_weights_equal"]
    out = _run(c)
    assert out["tree_edges"] == [(0, j) for j in range(1, 6)]
    assert out["rig_stats"][em.RIG_CENTER0] == 0 and out["tree"][:, 0].tolist() == [-1, 0, 0, 0, 0, 0]


def test_two_components():
    n = cases.named()
    out = _run(n["two_components_5_3"])
    rs = out["rig_stats"]
    assert rs[em.RIG_TREE_EDGES] == 6 and rs[em.RIG_NUM_CENTERS] in (1, 2) and rs[em.RIG_STATUS] & em.EST_UNREACHED and not rs[em.RIG_STATUS] & em.EST_ASSERT
    assert 0 < rs[em.RIG_REACHED] < 8
    not_reached = out["tree"][:, 0] == -2
    assert not_reached.sum() == 8 - rs[em.RIG_REACHED]
    assert all(np.array_equal(out["cameras"][i, 4:13], np.eye(3).ravel()) for i in np.where(not_reached)[0])
    out = _run(cases.make(8, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)], 31))           # two paths of 4: four centers, C:212 would assert
    rs = out["rig_stats"]
    assert rs[em.RIG_STATUS] & em.EST_ASSERT and rs[em.RIG_NUM_CENTERS] == 4 and rs[em.RIG_REACHED] == 0
    assert np.all(out["tree"] == [-2, -1]) and all(np.array_equal(out["cameras"][i, 4:13], np.eye(3).ravel()) for i in range(8))
    assert np.all(out["cameras"][:, 0] > 0)                                                    # the focals are still written


def test_focals_given_mode():
    c = cases.named()["focals_given"]
    out = _run(c)
    assert np.array_equal(out["cameras"][:, 0:2], c["focals_in"][:, 0:2]) and out["rig_stats"][em.RIG_CANDIDATES] == 0
    assert np.allclose(out["cameras"][:, 2:4], c["focals_in"][:, 2:4], rtol=0, atol=1e-9)      # - 0.5 w, + 0.5 w: two rounded operations
    assert out["rig_stats"][em.RIG_STATUS] == 0


def test_singular_h_gives_zeros_and_nans_not_errors():
    out = _run(cases.named()["singular_H"])
    assert out["rig_stats"][em.RIG_REACHED] == 4
    R = out["cameras"][:, 4:13]
    assert np.isnan(R).any() or (R == 0).all(axis=1).any()


def test_batched_equals_alone():
    n = cases.named()
    rigs = [n["demo_2_images_1_pair"], n["complete_5"], n["complete_9"]]
    j = cases.join(rigs)
    cams, kr, tree, rs = em.estimate(j["sizes"], j["pairs"], j["H"], j["stats"], j["rig_first"])
    at = 0
    for k, r in enumerate(rigs):
        o = _run(r)
        m = len(r["sizes"])
        assert np.array_equal(cams[at:at + m].view(np.uint64), o["cameras"].view(np.uint64)) and np.array_equal(tree[at:at + m], o["tree"])
        assert np.array_equal(rs[k], o["rig_stats"])
        at += m


def test_the_named_cases_are_what_their_names_say():
    NAMED = cases.named()

    def model(k):
        c = NAMED[k]
        return em.estimate(c["sizes"], c["pairs"], c["H"], c["stats"], c["rig_first"], c["focals_in"])
    rs = {k: model(k)[3][0] for k in NAMED if k != "complete_64"}
    rs["complete_64"] = model("complete_64")[3][0]
    for k in ("demo_2_images_1_pair", "chain_3", "complete_5", "complete_7", "complete_9", "complete_17", "complete_64", "all_weights_equal"):
        n = len(NAMED[k]["sizes"])
        assert rs[k][em.RIG_STATUS] == em.EST_MEDIAN and rs[k][em.RIG_REACHED] == n and rs[k][em.RIG_TREE_EDGES] == n - 1, k
        assert rs[k][em.RIG_CANDIDATES] == 2 * len(NAMED[k]["pairs"]), k
    assert rs["complete_64"][em.RIG_CANDIDATES] == 4032 and len(NAMED["complete_17"]["pairs"]) * 2 + 17 == 289
    assert rs["two_components_5_3"][em.RIG_STATUS] & em.EST_UNREACHED and rs["two_components_4_4"][em.RIG_STATUS] & (em.EST_ASSERT | em.EST_UNREACHED)
    assert rs["fallback_focal"][em.RIG_STATUS] == 0 and rs["fallback_focal"][em.RIG_CANDIDATES] == 0
    assert rs["focals_given"][em.RIG_STATUS] == 0
    cams = model("singular_H")[0]
    assert np.isnan(cams).any() or (cams[:, 4:13] == 0).all(axis=1).any()


def test_the_entry_is_declared():
    from imagestitch_amd import _lib, cameras
    assert {"isx_estimate_cameras", "isx_estimator_release"} <= set(_lib.declared_symbols())
    text = open(os.path.join(ROOT, "include", "imagestitch_hip.h")).read()
    for name, val in (("ISX_ESTIMATOR_MAX_IMAGES", em.MAX_IMAGES), ("ISX_ESTIMATOR_MEDIAN", em.EST_MEDIAN), ("ISX_ESTIMATOR_ASSERT", em.EST_ASSERT),
                      ("ISX_ESTIMATOR_UNREACHED", em.EST_UNREACHED)):
        assert "%s = %d" % (name, val) in text, name
    assert (cameras.MAX_IMAGES, cameras.ST_MEDIAN, cameras.ST_ASSERT, cameras.ST_UNREACHED) == (em.MAX_IMAGES, em.EST_MEDIAN, em.EST_ASSERT, em.EST_UNREACHED)


def test_fuzz_generator_covers_its_classes():
    """tools/fuzz_estimator.py without a GPU: every seeded class yields a valid call, the classes sit on the kernel's constants, and the
    share of pairs without H, of tied weights and of singular H are all exercised."""
    import fuzz_estimator as fz
    seen_n, seen_rigs, layouts, singular, no_h, ties = set(), set(), set(), 0, 0, 0
    for seed in range(len(fz.CLASSES) * 3):
        c = fz.make_case(seed)
        first = c["rig_first"] if c["rig_first"] is not None else [0, len(c["sizes"])]
        seen_rigs.add(len(first) - 1)
        seen_n |= {first[r + 1] - first[r] for r in range(len(first) - 1)}
        layouts.add(c["layout"])
        assert all(0 <= i < j < len(c["sizes"]) for i, j in c["pairs"]) and len(set(c["pairs"])) == len(c["pairs"])
        singular += c["singular"]
        no_h += int((c["stats"][:, 0] == 0).sum())
        w = c["stats"][c["stats"][:, 0] != 0, 1]
        ties += len(w) - len(set(w.tolist()))
        em.estimate(c["sizes"], c["pairs"], c["H"], c["stats"], c["rig_first"], c["focals_in"])      # the model runs on every case
    assert seen_n >= {2, 3, 8, 9, 16, 17, 63, 64}, seen_n
    assert seen_rigs >= {1, 2, 3, 4, 5} and layouts == {"host", "device", "strided"} and singular > 0 and no_h > 0 and ties > 0
