"""Times GainCompensator::feed (isx_gain_compensator_feed) on device-resident tiles, apart from bench.py:
  pair   config 2: two 3840 x 2160 tiles warped by the cylindrical warper (f = 3000, yaw 0.36), their warped masks
  mosaic 64 tiles of 3840 x 2160 in an 8 x 8 grid overlapping by 10 % on each side (all-255 masks)
For each: the whole call between two HIP events on its stream (it returns host values: table upload, the one launch, the partials'
download and the solve on the host), the kernel alone (its own start / end events, isx_profile_*), the bytes of the model
  bytes = sum_i mask_i + sum_{i<j, overlap} 8 overlap_px(i,j)
and the kernel's fraction of 8 TB/s.  One JSON line per workload."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imagestitch_amd as I  # noqa: E402
from imagestitch_amd import _lib, synth  # noqa: E402

PEAK = 8.0e12


def model_bytes(corners, sizes):
    total = sum(w * h for w, h in sizes)
    for i in range(len(sizes)):
        for j in range(i + 1, len(sizes)):
            w = min(corners[i][0] + sizes[i][0], corners[j][0] + sizes[j][0]) - max(corners[i][0], corners[j][0])
            h = min(corners[i][1] + sizes[i][1], corners[j][1] + sizes[j][1]) - max(corners[i][1], corners[j][1])
            if w > 0 and h > 0:
                total += 8 * w * h
    return total


def time_feed(name, corners, imgs, masks, iters, warmup):
    stream = torch.cuda.current_stream()
    comp = I.GainCompensator(stream=stream)
    for _ in range(warmup):
        comp.feed(corners, imgs, masks)
    lib = _lib.load()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call_ms = []
    for _ in range(iters):
        e0.record(stream)
        comp.feed(corners, imgs, masks)
        e1.record(stream)
        e1.synchronize()
        call_ms.append(e0.elapsed_time(e1))
    lib.isx_profile_enable(1)
    lib.isx_profile_reset()
    for _ in range(iters):
        comp.feed(corners, imgs, masks)
    ent = _lib.profile_entries()["gain_feed"]
    lib.isx_profile_enable(0)
    kern_us = ent["ms"] / ent["launches"] * 1e3
    sizes = [(m.shape[1], m.shape[0]) for m in masks]
    nbytes = model_bytes(corners, sizes)
    out = {"workload": name, "tiles": len(imgs), "call_us_median": round(float(np.median(call_ms)) * 1e3, 1),
           "kernel_us": round(kern_us, 2), "model_bytes": nbytes, "kernel_TBps": round(nbytes / (kern_us * 1e-6) / 1e12, 3),
           "kernel_frac_8TBps": round(nbytes / (kern_us * 1e-6) / PEAK, 3), "gains_head": [round(float(g), 6) for g in comp.gains()[:4]]}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["pair", "mosaic"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, F = 3840, 2160, 3000.0
    if a.only in (None, "pair"):
        K, Rs = synth.camera_pair(W, H, F)
        warper = I.CylindricalWarper().create(F)
        corners, imgs, masks = [], [], []
        for i in range(2):
            c, wi, wm = warper.warp_with_mask(torch.from_numpy(synth.make_tile(H, W, i)).to(dev), K, Rs[i])
            corners.append(c); imgs.append(wi); masks.append(wm)
        torch.cuda.synchronize()
        time_feed("config2_pair", corners, imgs, masks, a.iters, a.warmup)
        del imgs, masks
    if a.only in (None, "mosaic"):
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        corners, imgs, masks = [], [], []
        for r in range(8):
            for c in range(8):
                corners.append((c * (W - W // 10), r * (H - H // 10)))
                imgs.append(torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=gen))
                masks.append(torch.full((H, W), 255, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        time_feed("mosaic_64x4K", corners, imgs, masks, max(5, a.iters // 5), 2)


if __name__ == "__main__":
    main()
