"""Inputs of the homography tests: point sets (n x 4 float32: src.x, src.y, dst.x, dst.y) with a planted homography, the degenerate ones, sets
built from the sample stream so that the RANSAC loop ends or wins at a chosen iteration, and a seeded generator.  Every case is meant to
satisfy margin >= 1e-9 in the model (tests/test_homography_model.py checks it): its outcome does not hang on an ulp of pow / log."""
import numpy as np

from helpers import homography_np as hm

H_TRUE = np.array([[1.08, 0.03, 31.5], [-0.04, 0.97, -12.25], [2e-5, -3e-5, 1.0]])
SPAN = 400.0


def project(src, H=H_TRUE):
    q = np.c_[np.asarray(src, np.float64), np.ones(len(src))] @ H.T
    return q[:, :2] / q[:, 2:]


def planted(seed, n, inliers, noise=0.0):
    """n correspondences, the first `inliers` of a seeded shuffle follow H_TRUE (+ Gaussian noise in pixels), the rest are uniform."""
    r = np.random.default_rng(seed)
    src = r.uniform(-SPAN, SPAN, (n, 2)).astype(np.float32)
    dst = project(src) + r.normal(0.0, noise, (n, 2)) if noise else project(src)
    out = r.permutation(n)[inliers:]
    dst[out] = r.uniform(-SPAN, SPAN, (len(out), 2))
    return np.ascontiguousarray(np.c_[src, dst.astype(np.float32)], np.float32)


def exact(seed, n):
    """Every correspondence follows H_TRUE to float32 rounding: the first hypothesis takes all, ep = 0 ends the loop after iteration 1."""
    return planted(seed, n, n)


def collinear(n):
    """Every source point on the line y = 2 x (exact in float32): checkSubset refuses every subset, getSubset fails at iteration 0."""
    x = np.arange(n, dtype=np.float32) * 3 - 40
    src = np.c_[x, 2 * x]
    dst = np.random.default_rng(n).uniform(-SPAN, SPAN, (n, 2))
    return np.ascontiguousarray(np.c_[src, dst], np.float32)


def repeated(seed, distinct, copies):
    """`distinct` exact correspondences in general position, each `copies` times, shuffled: a subset with a repeated point is collinear."""
    base = exact(seed, distinct)
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(np.repeat(base, copies, 0)))


def all_the_same(n):
    """One correspondence n times: getSubset fails at iteration 0 after its 10000 attempts."""
    return np.tile(np.array([[3.0, 4.0, 5.0, 6.0]], np.float32), (n, 1))


def outliers(seed, n):
    r = np.random.default_rng(seed)
    return r.uniform(-SPAN, SPAN, (n, 4)).astype(np.float32)


def sparse_inliers(seed, n=40, inliers=16):
    """`inliers` of n correspondences follow H_TRUE exactly, the others are uniform: the first subset of inliers only takes the model's
    loop a while to draw."""
    r = np.random.default_rng(seed)
    pts = exact(seed, n)
    out = np.sort(r.permutation(n)[inliers:])
    pts[out, 2:4] = r.uniform(-SPAN, SPAN, (len(out), 2)).astype(np.float32)
    return pts


# (seed, inliers) of sparse_inliers found by running getSubset's stream: the first subset made of inliers only - the winning hypothesis - is
# that of iteration 63 (the last of the kernel's first chunk) and of iteration 64 (the first of its second); the tests assert both
WIN_AT = {63: (58, 16), 64: (1204, 14)}


def win_at(iteration):
    seed, inliers = WIN_AT[iteration]
    return sparse_inliers(seed, 40, inliers)


def inliers_for_iterations(target, n_range=range(12, 120)):
    """(n, inliers) for which RANSACUpdateNumIters1 gives `target` iterations with the comfortable margin the tests need."""
    for n in n_range:
        for good in range(5, n):
            m = []
            if hm.update_num_iters(0.995, float(n - good) / n, 4, 2000, m) == target and m[0] > 1e-4:
                return n, good
    raise AssertionError(target)


def stop_at(target, seed=0):
    """Exact inliers and uniform outliers in the proportion that ends the loop after `target` iterations."""
    n, good = inliers_for_iterations(target)
    return planted(seed + 100 * target, n, good)


def tiny_destinations(seed, n):
    """Destinations of order 1e-7: H is found, |det H| < DBL_EPSILON, and R:863 returns before the inliers are counted."""
    pts = exact(seed, n)
    pts[:, 2:4] *= np.float32(1e-9)
    return pts


def named():
    """name -> (points, keyword arguments of the call)."""
    c = {
        "n0": (np.zeros((0, 4), np.float32), {}),
        "n3_thresh1_3": (exact(3, 3), dict(num_matches_thresh1=3)),
        "n4_thresh1_4": (exact(4, 4), dict(num_matches_thresh1=4, num_matches_thresh2=4)),
        "n4_degenerate": (all_the_same(4), dict(num_matches_thresh1=4)),
        "n5_below_thresh1": (exact(5, 5), {}),
        "n5_thresh1_5": (exact(5, 5), dict(num_matches_thresh1=5, num_matches_thresh2=5)),
        "n6_exact": (exact(6, 6), {}),
        "n63_exact": (exact(63, 63), {}),
        "n64_exact": (exact(64, 64), {}),
        "n65_exact": (exact(65, 65), {}),
        "n300_exact": (exact(300, 300), {}),
        "n63_half_noisy": (planted(1063, 63, 32, 0.5), {}),
        "n64_half_noisy": (planted(1064, 64, 32, 0.5), {}),
        "n65_half_noisy": (planted(1065, 65, 33, 0.5), {}),
        "n300_half_noisy": (planted(1300, 300, 150, 0.5), {}),
        "collinear_40": (collinear(40), {}),
        "all_the_same_9": (all_the_same(9), {}),
        "repeated_5x4": (repeated(7, 5, 4), {}),
        "repeated_9x8": (repeated(8, 9, 8), {}),
        "outliers_to_the_end": (outliers(11, 50), dict(max_iters=70)),
        "outliers_one_chunk": (outliers(12, 30), dict(max_iters=64)),
        "stop_at_63": (stop_at(63), {}),
        "stop_at_64": (stop_at(64), {}),
        "stop_at_65": (stop_at(65), {}),
        "win_at_63": (win_at(63), {}),
        "win_at_64": (win_at(64), {}),
        "thresh_5px": (planted(21, 80, 50, 1.5), dict(reproj_thresh=5.0, confidence=0.99)),
        "thresh_default_when_negative": (planted(22, 40, 30, 0.3), dict(reproj_thresh=-1.0)),
        "degenerate_det": (tiny_destinations(31, 12), dict(reproj_thresh=1e-3)),
    }
    return c


def limits():
    """name -> points of tests/test_gpu_homography_limits.py: counts either side of two ballots of 64, 2 000 and 8 193 correspondences
    (the scoring loop, the compaction, pass 2 and the refit over thousands of rows), a half-outlier set of 4 096 (the iteration count
    shortens more than once) and the two exact sets either side of confidence > 3 -> 0: 240 / (8 + 0.3 * 240) = 3, 241 / 80.3 > 3.  The
    seeds are those at which tests/test_homography_model.py finds every margin >= 1e-6."""
    return {
        "n127_noisy": planted(2127, 127, 114, 0.2),
        "n128_noisy": planted(2128, 128, 115, 0.2),
        "n129_noisy": planted(2129, 129, 116, 0.2),
        "n2000_noisy": planted(4000, 2000, 1800, 0.3),
        "n8193_noisy": planted(10193, 8193, 7000, 0.3),
        "n4096_half_noisy": planted(6096, 4096, 2048, 0.5),
        "n240_exact": exact(2240, 240),
        "n241_exact": exact(2241, 241),
    }


def mixed_2016():
    """(point sets, the names of the distinct ones per set, keyword arguments) of one call of 2 016 pairs: 34 substantive sets - named ones
    and generated(0 .. 25) - at pairs 0, 255, 256, 257, 1 023, 2 015 and every 69th from 30, and between them, in turn, counts of 0, 1, 2
    and 3 (below num_matches_thresh1 = 4), the two n4 sets (runKernel over the four rows: one finds H, one does not), n5 (one pass) and
    n6_exact.  Sets that repeat are the same array, so a model run serves every place it stands at."""
    c = named()
    heavy = ["win_at_64", "n300_half_noisy", "collinear_40", "repeated_9x8", "outliers_to_the_end", "n65_half_noisy", "stop_at_64", "n64_exact"]
    sets = {k: c[k][0] for k in heavy}
    sets.update({"generated_%d" % i: generated(i) for i in range(26)})
    substantive = list(sets)
    light = ["n0", "n1", "n2", "n3", "n4_thresh1_4", "n4_degenerate", "n5_below_thresh1", "n6_exact"]
    sets.update({k: c[k][0] for k in light if k in c})
    sets.update({"n%d" % k: exact(3, 3)[:k] for k in (1, 2, 3)})
    at = [0, 255, 256, 257, 1023, 2015] + [30 + 69 * k for k in range(28)]
    assert len(set(at)) == len(at) == len(substantive) == 34 and max(at) == 2015
    names = [light[k % len(light)] for k in range(2016)]
    for k, name in zip(at, substantive):
        names[k] = name
    return sets, names, dict(num_matches_thresh1=4)


def generated(index):
    """Case `index` of the seeded generator: 6 - 300 correspondences, 30 - 90 % inliers, 0 - 1 px of noise."""
    r = np.random.default_rng(20261019 + index)
    n = int(r.integers(6, 301))
    frac = r.uniform(0.3, 0.9)
    return planted(50000 + index, n, max(int(round(frac * n)), min(n, 5)), float(r.uniform(0.0, 1.0)))
