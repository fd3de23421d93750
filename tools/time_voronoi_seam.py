"""Times VoronoiSeamFinder.find (isx_voronoi_seam_find) on device-resident masks, apart from bench.py, with DpSeamFinder.find and
GraphCutSeamFinder.find on the same inputs in the same run as the yardstick:
  ref    the reference's own warped tiles (CV_32FC3) with the masks that went into its seam finder (tests/golden/ref_dpseam_artifact.npz)
  pair4k config 2: two 3840 x 2160 tiles warped by the cylindrical warper (f = 3000), converted to CV_32FC3 as W:261 does
Two clocks for the Voronoi finder, which never synchronises: the host clock around find + a stream synchronise (median of --iters after
warm-up; the masks are restored from a device copy before each call, outside the timed span) and HIP events around --events calls
enqueued back to back (the calls after the first work on masks the first already cut: the same launches on the same cells).  The other
two finders synchronise by themselves and are timed on the host clock.  One JSON line per workload.  --only-voronoi skips the
yardsticks (for a profiler run)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imagestitch_amd as I  # noqa: E402
from imagestitch_amd import synth  # noqa: E402


def workloads():
    from test_ref_artifact import dpseam_case
    c = dpseam_case()
    yield "ref", c["corners"], [torch.from_numpy(a).cuda() for a in c["images"]], [torch.from_numpy(m).cuda() for m in c["masks_in"]]
    W, H, F = 3840, 2160, 3000.0
    K, Rs = synth.camera_pair(W, H, F)
    warper = I.CylindricalWarper().create(F)
    corners, imgs, masks = [], [], []
    for i in range(2):
        cc, wi, wm = warper.warp_with_mask(torch.from_numpy(synth.make_tile(H, W, 20 + i)).cuda(), K, Rs[i])
        corners.append(tuple(cc)); imgs.append(wi.float()); masks.append(wm)
    yield "pair4k", corners, imgs, masks


def host_clock(find, masks, warmup, iters):
    ts = []
    for k in range(warmup + iters):
        work = [m.clone() for m in masks]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        find(work)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            ts.append((t1 - t0) * 1e3)
    return round(float(np.median(ts)), 4), round(min(ts), 4), work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--events", type=int, default=100)
    ap.add_argument("--only-voronoi", action="store_true")
    a = ap.parse_args()
    for name, corners, imgs, masks in workloads():
        sizes = [(int(m.shape[1]), int(m.shape[0])) for m in masks]
        x0, y0 = max(corners[0][0], corners[1][0]), max(corners[0][1], corners[1][1])
        x1 = min(corners[0][0] + sizes[0][0], corners[1][0] + sizes[1][0])
        y1 = min(corners[0][1] + sizes[0][1], corners[1][1] + sizes[1][1])
        st = torch.cuda.current_stream()
        vor = I.VoronoiSeamFinder(stream=st)
        med, best, cut = host_clock(lambda w: vor.find(sizes, corners, w), masks, a.warmup, a.iters)
        work = [m.clone() for m in masks]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.events):
            vor.find(sizes, corners, work)
        e1.record()
        torch.cuda.synchronize()
        out = dict(workload=name, roi=[x1 - x0, y1 - y0], launches_per_pair=3, voronoi_ms_median=med, voronoi_ms_min=best,
                   voronoi_ms_events=round(e0.elapsed_time(e1) / a.events, 4), cleared=[int((m != c).sum()) for m, c in zip(masks, cut)])
        if not a.only_voronoi:
            dp = I.DpSeamFinder(stream=st)
            out["dp_ms_median"], out["dp_ms_min"], _ = host_clock(lambda w: dp.find(imgs, corners, w), masks, 1, a.iters)
            gc = I.GraphCutSeamFinder(stream=st)
            out["graphcut_ms_median"], out["graphcut_ms_min"], _ = host_clock(lambda w: gc.find(imgs, corners, w), masks, 1, a.iters)
        out["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
