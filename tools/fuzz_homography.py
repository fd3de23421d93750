"""Randomised parity of isx_find_homography against its NumPy model (tests/helpers/homography_np.py): masks and stats with np.array_equal,
H and conf through their uint64 views.

    python tools/fuzz_homography.py --seconds 600 --seed 20261201 [--out profiles/fuzz_homography_600s.json]
    python tools/fuzz_homography.py --refine --seconds 600 [--out profiles/fuzz_homography_lm_600s.json]

--refine runs the same cases through isx_find_homography_lm (the Levenberg-Marquardt polish, 12 stats columns) against
tests/helpers/homography_lm_np.py, with lm_max_iters drawn from 1, 2 and 10 by a generator of its own: case(seed, cls) is the same either way.

case(seed, cls) draws one of CLASSES (no GPU needed):
    tiny          4 .. 12 correspondences, the thresholds either side of the count
    chunk_edges   inliers in the proportion that ends the loop after 62 .. 66 iterations - either side of the kernel's chunk of 64
    count_limits  counts below, at and past the rows of the points and mask mats (clamped, status bit 3), negative counts
    noisy         13 .. 96 correspondences, 45 - 95 % inliers, 0 - 1 px of noise, thresholds and confidences drawn
    degenerate    collinear, repeated or identical points; pure outliers with a small max_iters
    multi         2 .. 5 pairs of the five classes above in one call
    large         400 .. 9 000 correspondences, 40 - 95 % inliers, 0 - 1 px of noise: scoring, compaction, pass 2 and the refit over thousands
                  of rows; drawn by a generator of its own, so that case(seed, cls) of the classes above is what it was before `large`
Layouts: host or device mats, points of 4 or 6 columns, masks of 1 or 3, spare rows past the count.
A case whose model margin is below 1e-9 is fragile (its outcome hangs on an ulp of pow / log): it is skipped and counted, and the run fails
when more than 1 % are."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import homography_cases as cases  # noqa: E402
from helpers import homography_lm_np as lm  # noqa: E402
from helpers import homography_np as hm  # noqa: E402

CLASSES = ("tiny", "chunk_edges", "count_limits", "noisy", "degenerate", "multi", "large")
SENT_I, SENT_F, SENT_B = -7777, -7777.25, 0xA5


def one(rng, cls):
    """(points, count, keyword arguments) of one pair."""
    s = int(rng.integers(1 << 30))
    kw = {}
    if cls == "tiny":
        n = int(rng.integers(4, 13))
        pts = cases.planted(s, n, int(rng.integers(min(n, 4), n + 1)), float(rng.choice([0.0, 0.3])))
        kw = dict(num_matches_thresh1=int(rng.integers(3, 8)), num_matches_thresh2=int(rng.integers(3, 8)))
        return pts, n, kw
    if cls == "chunk_edges":
        n, good = cases.inliers_for_iterations(int(rng.integers(62, 67)), range(int(rng.integers(12, 40)), 120))
        return cases.planted(s, n, good), n, kw
    if cls == "count_limits":
        n = int(rng.integers(6, 40))
        pts = cases.planted(s, n, max(n * 3 // 4, 5), 0.2)
        return pts, int(rng.choice([n - 1, n, n + 1, n + 9, -1, 0, 5, 6])), kw
    if cls == "noisy":
        n = int(rng.integers(13, 97))
        pts = cases.planted(s, n, max(int(n * rng.uniform(0.45, 0.95)), 6), float(rng.uniform(0.0, 1.0)))
        kw = dict(reproj_thresh=float(rng.choice([3.0, 1.5, 5.0, -1.0])), confidence=float(rng.choice([0.995, 0.99, 0.9])))
        return pts, n, kw
    if cls == "degenerate":
        kind = int(rng.integers(4))
        if kind == 0:
            pts = cases.collinear(int(rng.integers(6, 30)))
        elif kind == 1:
            pts = cases.repeated(s, int(rng.integers(5, 9)), int(rng.integers(2, 6)))
        elif kind == 2:
            pts = cases.all_the_same(int(rng.integers(6, 12)))
        else:
            pts, kw = cases.outliers(s, int(rng.integers(8, 50))), dict(max_iters=int(rng.integers(1, 80)))
        return pts, len(pts), kw
    if cls == "large":
        n = int(rng.integers(400, 9001))
        return cases.planted(s, n, int(n * rng.uniform(0.40, 0.95)), float(rng.uniform(0.0, 1.0))), n, kw
    raise ValueError(cls)


def case(seed, cls):
    """A call: per pair (points, count), shared keyword arguments, the layout."""
    rng = np.random.default_rng([int(seed), 0x4C47]) if cls == "large" else np.random.default_rng(seed)
    if cls == "multi":
        pairs = [one(rng, CLASSES[int(rng.integers(5))])[:2] for _ in range(int(rng.integers(2, 6)))]
        kw = {}
    else:
        pts, count, kw = one(rng, cls)
        pairs = [(pts, count)]
    return dict(pairs=pairs, kw=kw, device=bool(rng.integers(2)), wide=bool(rng.integers(2)), spare=int(rng.choice([0, 0, 3])))


def lm_iters_of(seed):
    """--refine: the case's lm_max_iters, from a generator that case() does not share."""
    return int(np.random.default_rng([int(seed), 0x4C4D]).choice([1, 2, 10]))


def expected(c, lm_max_iters=None):
    """The model's results, with the capacities of run_case's mats; lm_max_iters: those of the model with the polish."""
    if lm_max_iters is not None:
        return [lm.find_homography_lm_np(np.r_[p, np.zeros((c["spare"], 4), np.float32)], count=n, lm_max_iters=lm_max_iters, **c["kw"])
                for p, n in c["pairs"]]
    return [hm.find_homography_np(np.r_[p, np.zeros((c["spare"], 4), np.float32)], count=n, **c["kw"]) for p, n in c["pairs"]]


def run_case(c, want, lm_max_iters=None):
    """The library on the case's layout against `want`; returns the list of differences.  lm_max_iters: through isx_find_homography_lm."""
    import torch
    from imagestitch_amd import homography as hg
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if c["device"] else (lambda a: np.array(a))
    get = (lambda a: a.cpu().numpy()) if c["device"] else (lambda a: a)
    k = len(c["pairs"])
    ps, ms = [], []
    for p, _ in c["pairs"]:
        full = np.full((len(p) + c["spare"], 6 if c["wide"] else 4), SENT_F, np.float32)
        full[:, :4] = 0
        full[:len(p), :4] = p
        ps.append(put(full))
        ms.append(put(np.full((len(p) + c["spare"], 3 if c["wide"] else 1), SENT_B, np.uint8)))
    cnt = put(np.array([[n for _, n in c["pairs"]]], np.int32))
    H, st, cf = put(np.full((3 * k, 3), SENT_F, np.float64)), put(np.full((k, 8 if lm_max_iters is None else 12), SENT_I, np.int32)), put(np.full((1, k), SENT_F, np.float64))
    refine = {} if lm_max_iters is None else dict(refine=True, lm_max_iters=lm_max_iters)
    info = hg.find_homography(ps, cnt, H, ms, st, cf, **c["kw"], **refine)
    torch.cuda.synchronize()
    bad = [] if info == (k, 1) else ["info %s" % (info,)]
    Hh, sh, ch = get(H), get(st), get(cf)
    for i, w in enumerate(want):
        m = get(ms[i])
        n = 0 if w["mask"] is None else len(w["mask"])
        if not np.array_equal(sh[i], w["stats"]):
            bad.append("pair %d: stats %s, model %s" % (i, sh[i].tolist(), w["stats"].tolist()))
        if not np.array_equal(np.ascontiguousarray(Hh[3 * i:3 * i + 3]).view(np.uint64), w["H"].view(np.uint64)):
            bad.append("pair %d: H differs" % i)
        if np.float64(ch[0, i]).view(np.uint64) != np.float64(w["conf"]).view(np.uint64):
            bad.append("pair %d: conf differs" % i)
        if n and not np.array_equal(m[:n, 0], w["mask"]):
            bad.append("pair %d: mask differs" % i)
        if not (m[n:] == SENT_B).all() or not (m[:, 1:] == SENT_B).all():
            bad.append("pair %d: mask bytes past the count were written" % i)
    return bad


def scheduled(seed, n):
    """(case seed, class) of a soak's n-th case: the classes in turn."""
    return int(seed) * 1000003 + n, CLASSES[n % len(CLASSES)]


def run(seconds, seed, verbose=False, progress_path=None, refine=False):
    """Draws cases (the classes in turn) for `seconds` and compares the library with the model.  Returns a summary dict."""
    import torch
    import imagestitch_amd
    imagestitch_amd.load()
    t0 = time.time()
    per, failing, n, pairs, skipped, told = {c: 0 for c in CLASSES}, [], 0, 0, 0, t0
    while time.time() - t0 < seconds:
        if progress_path and time.time() - told >= 30.0:
            told = time.time()
            with open(progress_path, "w") as f:
                json.dump(dict(seconds=round(told - t0, 1), cases=n, mismatches=len(failing), skipped_fragile=skipped), f)
        s, cls = scheduled(seed, n)
        c = case(s, cls)
        iters = lm_iters_of(s) if refine else None
        want = expected(c, iters)
        n += 1
        per[cls] += 1
        if min(w["margin"] for w in want) < 1e-9:
            skipped += 1
            continue
        bad = run_case(c, want, iters)
        pairs += len(c["pairs"])
        if bad:
            failing.append(dict(seed=s, cls=cls, differences=bad[:4]))
            if verbose:
                print("MISMATCH", s, cls, bad[:4], flush=True)
    return dict(tool="fuzz_homography", refine=bool(refine), seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, pairs=pairs, mismatches=len(failing),
                skipped_fragile=skipped, too_many_fragile=bool(skipped > 0.01 * n), per_class=per, failing_seeds=failing[:20],
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261201)
    ap.add_argument("--out", default=None)
    ap.add_argument("--progress", default=None)
    ap.add_argument("--refine", action="store_true", help="isx_find_homography_lm against the model with the LM polish")
    a = ap.parse_args()
    out = run(a.seconds, a.seed, verbose=True, progress_path=a.progress, refine=a.refine)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(1 if out["mismatches"] or out["too_many_fragile"] else 0)


if __name__ == "__main__":
    main()
