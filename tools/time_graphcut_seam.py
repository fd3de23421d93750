"""Times GraphCutSeamFinder(cost).find (isx_graphcut_seam_find; --cost color, color_grad or both, one after the other on the same inputs in
the same run) on device-resident tiles, apart from bench.py:
  ref    the reference's own warped tiles (CV_32FC3) with the masks that went into its seam finder (tests/golden/ref_dpseam_artifact.npz)
  pair4k config 2: two 3840 x 2160 tiles warped by the cylindrical warper (f = 3000), converted to CV_32FC3 as W:261 does
  seam01 the same pair at seam_megapix 0.1: sources resized by sqrt(0.1e6 / (3840 * 2160)), K and the warper's scale times that factor
--certificate also checks the 64-bit certificate of every workload against the NumPy model's graph (tests/helpers/graphcut_grad_np.py).
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
    scale = float(np.sqrt(0.1e6 / (W * H)))
    Ks = K.copy()
    for r, c in ((0, 0), (0, 2), (1, 1), (1, 2)):
        Ks[r, c] = np.float32(Ks[r, c] * np.float32(scale))
    warper = I.CylindricalWarper().create(float(np.float32(F) * np.float32(scale)))
    corners, imgs, masks = [], [], []
    for i in range(2):
        small = I.resize(torch.from_numpy(synth.make_tile(H, W, 20 + i)).cuda(), fx=scale, fy=scale)
        cc, wi, wm = warper.warp_with_mask(small, Ks, Rs[i])
        corners.append(tuple(cc)); imgs.append(wi.float()); masks.append(wm)
    yield "seam01", corners, imgs, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cost", default="color", choices=["color", "color_grad", "both"])
    ap.add_argument("--workloads", default="ref,pair4k,seam01")
    ap.add_argument("--certificate", action="store_true")
    a = ap.parse_args()
    costs = ["color", "color_grad"] if a.cost == "both" else [a.cost]
    for name, corners, imgs, masks in workloads():
        if name not in a.workloads.split(","):
            continue
        for cost in costs:
            time_one(a, name, cost, corners, imgs, masks)


def check_certificate(cost_type, corners, imgs, masks, r):
    from helpers import graphcut_grad_np as GG
    from helpers import graphcut_np as G
    hi, hm = [x.cpu().numpy() for x in imgs], [m.cpu().numpy() for m in masks]
    roi = G.overlap_roi(corners[0], corners[1], (hi[0].shape[1], hi[0].shape[0]), (hi[1].shape[1], hi[1].shape[0]))
    G.check_certificate(GG.pair_graph(hi[0], hi[1], hm[0], hm[1], corners[0], corners[1], roi, cost_type), r["flow"], r["residuals"], r["labels"])


def time_one(a, name, cost, corners, imgs, masks):
    torch.cuda.synchronize()
    cost_type = I.seam.COST_COLOR_GRAD if cost == "color_grad" else I.seam.COST_COLOR
    finder = I.GraphCutSeamFinder(cost_type=cost_type, stream=torch.cuda.current_stream())
    work = [m.clone() for m in masks]
    info = finder.find_pair(imgs[0], imgs[1], corners[0], corners[1], work[0], work[1], certificate=a.certificate, wide=True)
    if a.certificate:
        check_certificate(cost_type, corners, imgs, masks, info)
    ts = []
    for k in range(a.warmup + a.iters):
        work = [m.clone() for m in masks]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        finder.find(imgs, corners, work)
        t1 = time.perf_counter()
        if k >= a.warmup:
            ts.append((t1 - t0) * 1e3)
    print(json.dumps(dict(workload=name, cost=cost, flow_scale=info["flow_scale"], certificate="ok" if a.certificate else None,
                          cleared=[int((w != m).sum()) for w, m in zip(work, masks)], grid=[info["rows"], info["cols"]], flow=info["flow"], rounds=info["rounds"],
                          launches=info["launches"], ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3),
                          device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
