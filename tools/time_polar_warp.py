"""The fused image + mask warp of one 4K tile (3840 x 2160, scale = f = 3000, yaw 0.36) through the fisheye and the stereographic projector
and, back to back in the same process, through the cylindrical one - the yardstick - and the ROI scan of the two new kinds alone (run on
the GPU box):

    python tools/time_polar_warp.py [--steps 50] [--warmup 10]

Every kind warps into its own ROI with isx_warper_warp_with_mask_roi (CV_8UC3 tile + all-255 mask, device mats; no ROI scan inside the timed
region).  `steps` warps are enqueued back to back between one pair of HIP events; five such rounds, the median.  The ROI scan is a
synchronous call (one launch, 16 bytes back, one stream synchronisation): its figure is the host's wall clock per call, alternating between
two cameras so that the handle's remembered answer never serves.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagestitch_amd as I  # noqa: E402
from imagestitch_amd import synth  # noqa: E402
from imagestitch_amd._lib import as_mat, check, f9  # noqa: E402


def measure(kind, img, K, R, F, steps, warmup):
    w = I.RotationWarper(kind, F)
    H, W = img.shape[:2]
    roi = w.warpRoi((W, H), K, R)
    dh, dw = roi[3] - roi[1] + 1, roi[2] - roi[0] + 1
    di = torch.empty((dh, dw, 3), dtype=torch.uint8, device=img.device)
    dm = torch.empty((dh, dw), dtype=torch.uint8, device=img.device)
    mi, mdi, mdm, Kp, Rp, rc = as_mat(img), as_mat(di), as_mat(dm), f9(K), f9(R), (C.c_int * 4)(*roi)

    def step():
        check(w._lib.isx_warper_warp_with_mask_roi(w._h, C.byref(mi), None, Kp[1], Rp[1], rc, C.byref(mdi), C.byref(mdm)))

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / steps)
    med = float(np.median(us))
    return {"us_per_warp_median": round(med, 2), "us_per_warp_min": round(float(min(us)), 2), "warped_size": [dw, dh], "ns_per_warped_pixel": round(med * 1e3 / (dw * dh), 5)}


def measure_roi(kind, size, K, Rs, F, calls):
    w = I.RotationWarper(kind, F)
    for R in Rs:
        w.warpRoi(size, K, R)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        for i in range(calls):
            w.warpRoi(size, K, Rs[i & 1])
        t.append((time.perf_counter() - t0) / calls * 1e6)
    return {"us_per_call_median": round(float(np.median(t)), 2), "us_per_call_min": round(float(min(t)), 2), "source_pixels": size[0] * size[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    W, H, F = 3840, 2160, 3000.0
    K, Rs = synth.camera_pair(W, H, F)
    img = torch.from_numpy(synth.make_tile(H, W, 1)).cuda()
    out = {"tool": "time_polar_warp", "device": torch.cuda.get_device_name(0), "source": [W, H], "scale": F, "steps": a.steps}
    for name in ("cylindrical", "fisheye", "stereographic", "cylindrical"):          # the yardstick before and after
        key = name if name not in out else name + "_again"
        out[key] = measure(name, img, K, Rs[1], F, a.steps, a.warmup)
    for name in ("fisheye", "stereographic"):
        out[name]["ratio_to_cylindrical"] = round(out[name]["ns_per_warped_pixel"] / out["cylindrical"]["ns_per_warped_pixel"], 2)
        out["roi_" + name] = measure_roi(name, (W, H), K, Rs, F, 20)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
