"""Times BestOf2NearestMatcher's two entries (isx_match_features, then isx_find_homography on its points and counts) on device-resident
features, apart from bench.py:
  pair2k   2 images x 2 000 rows (1 pair)
  ring8    8 images x 2 000 rows (28 pairs)
Every image holds --shared keypoints of one scene under a planted homography (descriptors a bit apart) among random rows, so that each pair
has a few hundred matches with outliers among them.  Two clocks, since neither call synchronises on device mats: the host clock around the
chained calls + a stream synchronise (median and minimum of --iters after --warmup) and HIP events around --events chained calls enqueued
back to back; the homography entry alone is timed the same way on the matcher's outputs.  One JSON line per workload.  --refine times
isx_find_homography_lm (the Levenberg-Marquardt polish) in the homography entry's place."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from imagestitch_amd import homography, matcher  # noqa: E402

H_STEP = np.array([[1.02, 0.01, 14.0], [-0.012, 0.99, -6.5], [4e-6, -6e-6, 1.0]])


def features(seed, images, rows, shared):
    r = np.random.default_rng(seed)
    base_kp = r.uniform(-300, 300, (shared, 2))
    base_d = r.integers(0, 256, (shared, 32), dtype=np.uint8)
    descs, kps = [], []
    H = np.eye(3)
    for i in range(images):
        d = r.integers(0, 256, (rows, 32), dtype=np.uint8)
        kp = r.uniform(-380, 380, (rows, 2))
        d[:shared] = base_d
        flips = r.integers(0, 256, (shared, 3))                       # three flipped bits an image
        for f in flips.T:
            d[np.arange(shared), f // 8] ^= (1 << (f % 8)).astype(np.uint8)
        q = np.c_[base_kp, np.ones(shared)] @ H.T
        kp[:shared] = q[:, :2] / q[:, 2:] + r.normal(0, 0.4, (shared, 2))
        perm = r.permutation(rows)
        descs.append(torch.from_numpy(np.ascontiguousarray(d[perm])).cuda())
        kps.append(torch.from_numpy(np.ascontiguousarray((kp[perm] + [400, 300]).astype(np.float32))).cuda())
        H = H_STEP @ H
    return descs, kps, [(800, 600)] * images


def clocks(fn, a):
    ts = []
    for k in range(a.warmup + a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= a.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.events):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(float(np.median(ts)), 4), round(min(ts), 4), round(e0.elapsed_time(e1) / a.events, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--shared", type=int, default=400)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=50)
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--lm-max-iters", type=int, default=10)
    a = ap.parse_args()
    st = torch.cuda.current_stream()
    for name, n in (("pair2k", 2), ("ring8", 8)):
        descs, kps, sizes = features(n, n, a.rows, a.shared)
        pairs = [(i, j) for i in range(n - 1) for j in range(i + 1, n)]
        k = len(pairs)
        dev = dict(device="cuda")
        ms = [torch.empty((2 * a.rows, 3), dtype=torch.int32, **dev) for _ in pairs]
        ps = [torch.empty((2 * a.rows, 4), dtype=torch.float32, **dev) for _ in pairs]
        masks = [torch.empty((2 * a.rows, 1), dtype=torch.uint8, **dev) for _ in pairs]
        cnt = torch.empty((1, k), dtype=torch.int32, **dev)
        H, stats = torch.empty((3 * k, 3), dtype=torch.float64, **dev), torch.empty((k, 12 if a.refine else 8), dtype=torch.int32, **dev)
        conf = torch.empty((1, k), dtype=torch.float64, **dev)

        def match():
            return matcher.match_features(descs, pairs, 0.3, ms, cnt, kps, sizes, ps, stream=st)

        def homog():
            return homography.find_homography(ps, cnt, H, masks, stats, conf, stream=st, refine=a.refine, lm_max_iters=a.lm_max_iters)

        def both():
            match()
            return homog()
        info = both()
        chained, alone, matching = clocks(both, a), clocks(homog, a), clocks(match, a)
        s = stats.cpu().numpy()
        lm_cols = dict(refine=True, lm_max_iters=a.lm_max_iters, lm_iterations=[[int(v) for v in r] for r in s[:4, 8:12]]) if a.refine else {}
        print(json.dumps(dict(workload=name, **lm_cols, images=n, rows=a.rows, pairs=k, launches_homography=info[1],
                              chained_ms=dict(median=chained[0], min=chained[1], events=chained[2]),
                              homography_ms=dict(median=alone[0], min=alone[1], events=alone[2]),
                              match_ms=dict(median=matching[0], min=matching[1], events=matching[2]),
                              matches=[int(v) for v in cnt.cpu().numpy()[0][:4]], inliers=[int(v) for v in s[:4, 1]],
                              iterations_pass1=[int(v) for v in s[:4, 2]], max_iterations_pass1=int(s[:, 2].max()), status=sorted(set(int(v) for v in s[:, 0])),
                              device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
