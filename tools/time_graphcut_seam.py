"""Times GraphCutSeamFinder(COST_COLOR).find (isx_graphcut_seam_find) on device-resident tiles, apart from bench.py:
  ref    the reference's own warped tiles (CV_32FC3) with the masks that went into its seam finder (tests/golden/ref_dpseam_artifact.npz)
  pair4k config 2: two 3840 x 2160 tiles warped by the cylindrical warper (f = 3000), converted to CV_32FC3 as W:261 does
The call synchronises its stream (it reads an active-node count back every round), so it is timed on the host clock, masks restored
from a device copy before every call.  For each workload one JSON line: the padded grid, the maximum flow, the push-relabel rounds and
kernel launches of the pair (the one-pair form), and the median / min time per find over --iters calls."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    for name, corners, imgs, masks in workloads():
        torch.cuda.synchronize()
        finder = I.GraphCutSeamFinder(stream=torch.cuda.current_stream())
        work = [m.clone() for m in masks]
        info = finder.find_pair(imgs[0], imgs[1], corners[0], corners[1], work[0], work[1])
        ts = []
        for k in range(a.warmup + a.iters):
            work = [m.clone() for m in masks]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            finder.find(imgs, corners, work)
            t1 = time.perf_counter()
            if k >= a.warmup:
                ts.append((t1 - t0) * 1e3)
        print(json.dumps(dict(workload=name, grid=[info["rows"], info["cols"]], flow=info["flow"], rounds=info["rounds"],
                              launches=info["launches"], ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3),
                              device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
