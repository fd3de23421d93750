"""The batched tile warp of a config-2-sized pair (2 x 3840 x 2160, scale = f = 3000, yaw -/+ 0.36) through the plane projector, beside the
cylindrical warp of the same sources (run on the GPU box):

    python tools/time_plane_warp.py [--steps 200] [--warmup 20]

The two planned warps of a step (ISX_8UC3 tile + all-255 mask) leave as ONE launch (begin_batch .. end_batch).  `steps` steps are enqueued
back to back between one pair of HIP events, so the stream stays busy and the quotient is the launch's time, not the host's issue latency
(the host's own time to enqueue a step is printed beside it: where it exceeds the GPU time per step the figure is host-bound; the kernel's
own duration is in the rocprofv3 kernel trace of the same command).  Five such rounds; the median.  Both kinds run with deferred
verification and drop it (the ROI check is not what is timed); one verified step at the end proves the plan.  Bytes by the model of
SURVEY §8(d): 3 s + 4 n per tile (s source pixels read as CV_8UC3, n warped pixels written as CV_8UC3 + CV_8U), as a fraction of 8 TB/s.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagestitch_amd as I  # noqa: E402
from imagestitch_amd import synth  # noqa: E402

PEAK = 8e12


def pitched(h, row_bytes, shape, strides, dev):
    pitch = (row_bytes + 63) // 64 * 64
    return torch.empty((h * pitch,), dtype=torch.uint8, device=dev).as_strided(shape, (pitch,) + strides)


def measure(creator, imgs, K, Rs, F, steps, warmup, dev):
    w = creator().create(F)
    H, W = imgs[0].shape[:2]
    rois = [w.warpRoi((W, H), K, R) for R in Rs]
    sizes = [(r[2] - r[0] + 1, r[3] - r[1] + 1) for r in rois]
    outs = [(pitched(h, ww * 3, (h, ww, 3), (3, 1), dev), pitched(h, ww, (h, ww), (1,), dev)) for ww, h in sizes]

    def step():
        w.begin_batch()
        for i in range(len(imgs)):
            w.warp_with_mask_planned(imgs[i], K, Rs[i], rois[i], outs[i][0], outs[i][1])
        w.end_batch()

    w.set_deferred_verify(True)          # the same for both kinds: no verification inside the timed region
    for _ in range(warmup):
        step()
        w.discard_pending()
    torch.cuda.synchronize()
    us, host_us = [], []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
            w.discard_pending()
        host_us.append((time.perf_counter() - t0) / steps * 1e6)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / steps)
    step()
    w.verify()
    assert w.plan_status() == 0
    n = sum(ww * h for ww, h in sizes)
    nbytes = 3 * W * H * len(imgs) + 4 * n
    med = float(np.median(us))
    return {"us_per_step_median": round(med, 2), "us_per_step_min": round(float(min(us)), 2), "host_issue_us_per_step": round(float(np.median(host_us)), 2),
            "warped_pixels": int(n), "model_bytes": int(nbytes), "ns_per_warped_pixel": round(med * 1e3 / n, 5),
            "fraction_of_8TBps": round(nbytes / (med * 1e-6) / PEAK, 4), "sizes": sizes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, F = 3840, 2160, 3000.0
    K, Rs = synth.camera_pair(W, H, F)
    imgs = [torch.from_numpy(synth.make_tile(H, W, i)).to(dev) for i in range(2)]
    res = {"gpu": torch.cuda.get_device_name(0), "steps": a.steps, "source": [W, H], "scale": F}
    # alternate the two kinds twice: a drift of the box shows as a difference between a kind's two legs
    for leg in range(2):
        for name, creator in (("cylindrical", I.CylindricalWarper), ("plane", I.PlaneWarper)):
            res["%s_%d" % (name, leg)] = measure(creator, imgs, K, Rs, F, a.steps, a.warmup, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
