"""Times BlocksGainCompensator (isx_blocks_gain_feed / isx_blocks_gain_apply) on device-resident tiles, apart from bench.py.  One JSON line each:

  feed    the whole call and its stages (statistics, assembly, LU, back substitution: the host's clock around work that ends in a stream
          synchronise, isx_blocks_gain_feed_times), median of --iters, for
            ref_1101    two 1101 x 1101 tiles at dx = 799 (the reference's tile geometry), 32 x 32 blocks: 2 450 unknowns
            4k_64       two 3840 x 2160 tiles overlapping by a quarter, 64 x 64 blocks: 4 080 unknowns
            4k_32       the same at 32 x 32: 16 320 unknowns, a 2.1 GB matrix - ONCE, only with --big (give the command a time limit)
  host_lu the scalar lu_solve that isx_gain_compensator_feed solves with, on the assembled 2 450-unknown system, once, beside the device's
  apply   isx_blocks_gain_apply against isx_gain_apply on one 4K tile, alternating in one process, HIP events around --reps calls each,
          median of --iters: both move 6 B per pixel; the goal is within 1.25 x."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imagestitch_amd as I  # noqa: E402
from imagestitch_amd import exposure  # noqa: E402

ALPHA, BETA = 0.01, 100.0


def pair(w, h, dx, seed):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    base = torch.randint(0, 200, (h, w + dx, 3), dtype=torch.uint8, device=dev, generator=gen)
    t0 = base[:, :w].contiguous()
    t1 = torch.clamp(base[:, dx:].to(torch.int32) * 5 // 4 + 10, 0, 255).to(torch.uint8).contiguous()
    mask = torch.full((h, w), 255, dtype=torch.uint8, device=dev)
    return [(0, 0), (dx, 0)], [t0, t1], [mask, mask]


def time_feed(name, corners, imgs, masks, bl, iters, warmup):
    comp = I.BlocksGainCompensator(bl, bl)
    for _ in range(warmup):
        comp.feed(corners, imgs, masks)
    calls, stages = [], []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        comp.feed(corners, imgs, masks)
        calls.append((time.perf_counter() - t) * 1e3)
        stages.append(comp.feed_times())
    g = comp.gains()
    out = {"workload": name, "blocks": bl, "unknowns": int(g.size), "matrix_MB": round(g.size * (g.size + 1) * 8 / 1e6, 1), "iters": iters,
           "call_ms_median": round(float(np.median(calls)), 3), "gains_min_max": [round(float(g.min()), 6), round(float(g.max()), 6)]}
    for k in stages[0]:
        out[k + "_ms_median"] = round(float(np.median([s[k] for s in stages])), 3)
    print(json.dumps(out), flush=True)
    return comp


def dense_system(comp):
    pairs, diag = comp.block_stats()
    n = diag.size
    A = np.zeros((n, n))
    b = np.zeros(n)
    adj = [[(i, float(diag[i]), 0.0, 0.0)] for i in range(n)]
    for i, j, c, iij, iji in pairs.tolist():
        adj[i].append((j, float(c), iij, iji))
        adj[j].append((i, float(c), iji, iij))
    for i in range(n):
        for j, c, iij, iji in sorted(adj[i]):
            b[i] += BETA * c
            A[i, i] += BETA * c
            if j != i:
                A[i, i] += 2 * ALPHA * iij * iij * c
                A[i, j] -= 2 * ALPHA * iij * iji * c
    return A, b


def time_host_lu(comp):
    A, b = dense_system(comp)
    t = time.perf_counter()
    xh, _ = exposure.lu_solve(A, b, where="host")
    host_ms = (time.perf_counter() - t) * 1e3
    exposure.lu_solve(A, b)                                        # warm
    t = time.perf_counter()
    xd, swaps = exposure.lu_solve(A, b)
    dev_ms = (time.perf_counter() - t) * 1e3
    print(json.dumps({"workload": "host_lu_vs_device", "unknowns": int(b.size), "host_lu_solve_ms": round(host_ms, 1),
                      "device_selftest_ms_with_upload": round(dev_ms, 1), "swaps": swaps,
                      "max_rel_diff_host_device": float(np.max(np.abs(xh - xd) / np.abs(xh))),
                      "max_rel_diff_device_feed": float(np.max(np.abs(comp.gains() - xd) / np.abs(xd)))}), flush=True)


def time_apply(iters, reps):
    corners, imgs, masks = pair(3840, 2160, 2880, 3)
    comp = I.BlocksGainCompensator().feed(corners, imgs, masks)
    tile = imgs[0].clone()
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(fn):
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def blocks():
        comp.apply(0, corners[0], tile)

    def scalar():
        I.gain_apply(tile, 1.0009765625)
    for _ in range(3):
        run(blocks); run(scalar)
    a, b = [], []
    for _ in range(iters):                                         # alternating
        tile.copy_(imgs[0])
        a.append(run(blocks))
        tile.copy_(imgs[0])
        b.append(run(scalar))
    ma, mb = float(np.median(a)), float(np.median(b))
    px = 3840 * 2160
    print(json.dumps({"workload": "apply_4k_tile", "reps": reps, "iters": iters, "blocks_gain_apply_us": round(ma, 2), "gain_apply_us": round(mb, 2),
                      "ratio": round(ma / mb, 3), "goal": 1.25, "blocks_gain_apply_TBps": round(6.0 * px / (ma * 1e-6) / 1e12, 3),
                      "gain_apply_TBps": round(6.0 * px / (mb * 1e-6) / 1e12, 3),
                      "spread_us": [round(float(np.min(a)), 2), round(float(np.max(a)), 2), round(float(np.min(b)), 2), round(float(np.max(b)), 2)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big", action="store_true", help="also the 4K pair at 32 x 32 (16 320 unknowns), once")
    ap.add_argument("--only", choices=["feed", "apply", "big"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.only in (None, "feed"):
        comp = time_feed("ref_1101", *pair(1101, 1101, 799, 1), 32, a.iters, 1)
        time_host_lu(comp)
        time_feed("4k_64", *pair(3840, 2160, 2880, 2), 64, a.iters, 1)
    if a.only in (None, "apply"):
        time_apply(a.iters, a.reps)
    if a.big or a.only == "big":
        time_feed("4k_32", *pair(3840, 2160, 2880, 2), 32, 1, 0)


if __name__ == "__main__":
    main()
