"""Times the stages of seam finding at reduced scale on device-resident mats, apart from bench.py, on config 2 (two 3840 x 2160 tiles,
cylindrical warper, f = 3000) at --seam-megapix (0.1, OpenCV's default):
  dilate_resize_and   isx_mask_dilate_resize_and(small seam mask, full warped mask, 3 x 3), with the parent's isx_mask_dilate_and (3 x 3) on the
                      same full-size mats in the same run as the yardstick: both read the warped mask once and write the output once
  resize              isx_resize: the 4K CV_8UC3 source to seam scale (LINEAR), and the seam-scale CV_8UC1 mask to the warped tile's size
  finders             GraphCutSeamFinder.find and DpSeamFinder.find (and VoronoiSeamFinder.find) on the pair warped at seam scale
The kernels are timed between HIP events around --events calls enqueued back to back after a warm-up (no call synchronises on device mats);
rates are the algorithmic bytes (computed here from the shapes) over that time, against 8 TB/s.  The finders synchronise by themselves and
are timed on the host clock, median of --iters after a warm-up, the masks restored from a device copy before each call outside the timed
span (as tools/time_graphcut_seam.py does).  One JSON line per stage."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imagestitch_amd as I  # noqa: E402
from imagestitch_amd import synth  # noqa: E402

PEAK = 8.0e12


def events(fn, n, warmup=10):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


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


def rate(ms, nbytes):
    bps = nbytes / (ms * 1e-3)
    return dict(ms=round(ms, 5), alg_bytes=int(nbytes), tb_per_s=round(bps / 1e12, 4), of_8_tb_per_s=round(bps / PEAK, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seam-megapix", type=float, default=0.1)
    ap.add_argument("--events", type=int, default=100)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-finders", action="store_true")
    a = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    W, H, F = 3840, 2160, 3000.0
    K, Rs = synth.camera_pair(W, H, F)
    scale = min(1.0, float(np.sqrt(a.seam_megapix * 1e6 / (W * H))))
    imgs = [torch.from_numpy(synth.make_tile(H, W, 20 + i)).cuda() for i in range(2)]
    warper = I.CylindricalWarper().create(F)
    Ks = K.copy()
    for r, c in ((0, 0), (0, 2), (1, 1), (1, 2)):
        Ks[r, c] = np.float32(Ks[r, c] * np.float32(scale))
    small_warper = I.CylindricalWarper().create(float(np.float32(F) * np.float32(scale)))
    small = [I.resize(im, fx=scale, fy=scale) for im in imgs]
    corners, wmasks, sc, simg, smask = [], [], [], [], []
    for i in range(2):
        c, _, wm = warper.warp_with_mask(imgs[i], K, Rs[i])
        corners.append(tuple(c)); wmasks.append(wm)
        c, wi, wm = small_warper.warp_with_mask(small[i], Ks, Rs[i])
        sc.append(tuple(c)); simg.append(wi); smask.append(wm)
    torch.cuda.synchronize()
    geom = dict(seam_scale=round(scale, 6), source=[W, H], small_source=[int(small[0].shape[1]), int(small[0].shape[0])],
                warped=[int(wmasks[0].shape[1]), int(wmasks[0].shape[0])], small_warped=[int(smask[0].shape[1]), int(smask[0].shape[0])], device=dev)

    # the mask stage against the plain 3 x 3 dilate & AND on the same full-size mats
    seam_small = [m.clone() for m in smask]
    I.VoronoiSeamFinder().find(simg, sc, seam_small)
    full, out = wmasks[0], torch.empty_like(wmasks[0])
    n = full.shape[0] * full.shape[1]
    seam_full = I.dilate_resize_and(seam_small[0], full, 3, 3)             # a full-size seam mask for the yardstick to dilate
    lib, as_mat = I._lib.load(), I._lib.as_mat
    ms, mm, mt, mo = as_mat(seam_small[0]), as_mat(seam_full), as_mat(full), as_mat(out)

    def new():
        I._lib.check(lib.isx_mask_dilate_resize_and(C.byref(ms), C.byref(mt), 3, 3, C.byref(mo), 0, None))

    def old():
        I._lib.check(lib.isx_mask_dilate_and(C.byref(mm), C.byref(mt), 3, 3, C.byref(mo), 0, None))
    t_new = events(new, a.events)
    t_old = events(old, a.events)
    t_new2 = events(new, a.events)
    t_old2 = events(old, a.events)
    # the kernels' own begin-to-end times (the library's per-launch events), which leave out the launch gaps of a 4 us kernel
    lib.isx_profile_enable(1); lib.isx_profile_reset()
    for _ in range(a.events):
        new(); old()
    torch.cuda.synchronize()
    prof = I._lib.profile_entries()
    lib.isx_profile_enable(0)
    kern = {k: round(v["ms"] / max(v["launches"], 1), 5) for k, v in prof.items() if k in ("dilate_resize_and", "dilate_and")}
    print(json.dumps(dict(stage="dilate_resize_and", **geom, calls=a.events, new=rate(t_new, 2 * n), new_again=rate(t_new2, 2 * n), dilate_and_3x3=rate(t_old, 2 * n),
                          dilate_and_3x3_again=rate(t_old2, 2 * n), ratio=round(min(t_new, t_new2) / min(t_old, t_old2), 3), kernel_ms=kern,
                          kernel_ratio=round(kern["dilate_resize_and"] / kern["dilate_and"], 3) if len(kern) == 2 else None)), flush=True)

    # isx_resize
    dst = torch.empty_like(small[0])
    t = events(lambda: I.resize(imgs[0], (dst.shape[1], dst.shape[0]), dst=dst), a.events)
    print(json.dumps(dict(stage="resize_8uc3_4k_to_seam_scale_linear", **geom, **rate(t, 3 * (W * H + dst.shape[0] * dst.shape[1])))), flush=True)
    up = torch.empty_like(full)
    t = events(lambda: I.resize(seam_small[0], (up.shape[1], up.shape[0]), dst=up), a.events)
    print(json.dumps(dict(stage="resize_8uc1_seam_scale_to_warped_tile_linear", **geom, **rate(t, n + seam_small[0].numel()))), flush=True)

    if not a.skip_finders:
        st = torch.cuda.current_stream()
        f32 = [w.float() for w in simg]
        res = dict(stage="finders_at_seam_scale", **geom, full_scale_recorded_ms=dict(graphcut=2070.0, dp=66.9))
        gc, dp, vor = I.GraphCutSeamFinder(stream=st), I.DpSeamFinder(stream=st), I.VoronoiSeamFinder(stream=st)
        res["graphcut_ms_median"], res["graphcut_ms_min"], cut = host_clock(lambda w: gc.find(f32, sc, w), smask, 1, a.iters)
        res["graphcut_cleared"] = [int((m != c).sum()) for m, c in zip(smask, cut)]
        res["dp_ms_median"], res["dp_ms_min"], _ = host_clock(lambda w: dp.find(f32, sc, w), smask, 1, a.iters)
        res["voronoi_ms_median"], res["voronoi_ms_min"], _ = host_clock(lambda w: vor.find(simg, sc, w), smask, 1, a.iters)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
