"""Randomised parity of the fisheye and stereographic projectors (ISX_WARP_FISHEYE, ISX_WARP_STEREOGRAPHIC) against their NumPy model
(tests/helpers/polar_np.py): detectResultRoi, buildMaps, warp and the fused image + mask warp with np.array_equal.

    python tools/fuzz_polar_warp.py --seconds 600 --seed 20261020 [--out profiles/fuzz_polar_warp_600s.json]

The generator (no GPU needed: tests/test_polar_fuzz_generator.py checks it).  case(seed) draws one of CLASSES, each for either kind:
    rigs          one of the suite's rigs (identity, yaw 0.52 / 2.97, pitch +-pi/3, +-pi/2) with a random perturbation of up to 0.05 rad an axis
                  and of the focal length and principal point - the poles and the antipoles stay inside or next to the destination
    tile_edges    source and window sizes at a multiple of the kernels' tiling constants (64 x 4 destination pixels a block, 256 x 16
                  source pixels a block of the ROI scan), one less, one more
    pole_window   a window around the destination origin (r = 0: atan2f(0, 0), 1.f / 0, atanf(inf))
    far_window    a window far outside the image's ROI: r up to 2^31 / scale, beyond the 2^28 at which sinf / cosf give NaN
    fused         warp_with_mask: with or without a source mask, CV_8UC3 or CV_16SC3, with or without a gain
    captured      buildMaps, warp or the fused warp over a given window on device mats, captured ONCE into a hipGraph on a side stream; the
                  source (and the source mask) is then overwritten in place, the destinations are cleared, and the REPLAY is compared with
                  the model on the new bytes
Every case draws the entry (roi, maps, warp, fused), the pixel type, interpolation (NEAREST, LINEAR, LINEAR | TIES_EVEN), border mode and
layout (host mats, device tensors, rows that are views into wider mats).  A rig whose ROI exceeds FULL_WARP_PIXELS is warped through a
window only (tests/polar_cases.py: window_of)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import polar_cases as PC  # noqa: E402
from helpers import polar_np as P  # noqa: E402

CLASSES = ("rigs", "tile_edges", "pole_window", "far_window", "fused", "captured")
ENTRIES = ("roi", "maps", "warp", "fused")
TYPES = ((3, "uint8"), (1, "uint8"), (3, "float32"), (1, "float32"))
INTERPS = (PC.NEAREST, PC.LINEAR, PC.LINEAR | PC.TIES_EVEN)
BORDERS = (PC.CONST, PC.REPL, PC.REFLECT, PC.WRAP, PC.REFLECT101)
LAYOUTS = ("host", "device", "strided")
COL_BLOCK, ROW_BLOCK, SCAN_COLS, SCAN_ROWS = 64, 4, 256, 16
MAX_WINDOW = 160


def _rot3(yaw, pitch, roll):
    cz, sz = np.cos(roll), np.sin(roll)
    return P.rot("y", yaw) @ P.rot("x", pitch) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)


def _edge(rng, unit, most=2):
    return max(1, int(rng.integers(1, most + 1)) * unit + int(rng.integers(-1, 2)))


def case(seed, cls=None):
    """One case as a dict of plain values and arrays: kind, cls, w, h, scale, K, R, entry, cn, dtype, interp, border, layout, window (None:
    the rig's ROI, or its window_of where that is blown up), with_mask, out16, gain, img_seed."""
    rng = np.random.default_rng(int(seed))
    cls = cls or CLASSES[int(rng.integers(0, len(CLASSES)))]
    kind = int(rng.choice([P.FISHEYE, P.STEREOGRAPHIC]))
    names = list(P.ROTATIONS)
    rname = names[int(rng.integers(0, len(names)))]
    w, h = int(rng.integers(3, 200)), int(rng.integers(3, 120))
    if cls == "tile_edges":
        w, h = _edge(rng, SCAN_COLS if rng.random() < 0.3 else COL_BLOCK, 1 if rng.random() < 0.5 else 3), _edge(rng, SCAN_ROWS if rng.random() < 0.5 else ROW_BLOCK, 6)
    if cls == "far_window" and rng.random() < 0.4:          # a tiny source has a small scale: r = 2^31 / scale then passes 2^28
        w, h = int(rng.integers(3, 7)), int(rng.integers(3, 7))
    f = float(rng.uniform(0.5, 1.6) * max(w, h))
    amp = 0.05
    R = (P.ROTATIONS[rname] @ _rot3(*rng.uniform(-amp, amp, 3))).astype(np.float32)
    K = np.array([[f, 0, w / 2 + rng.uniform(-2, 2)], [0, f * rng.uniform(0.97, 1.03), h / 2 + rng.uniform(-2, 2)], [0, 0, 1]], np.float32)
    scale = float(np.float32(f * rng.uniform(0.8, 1.25)))
    entry = "fused" if cls == "fused" else ENTRIES[int(rng.integers(0, 3))]
    window = None
    if cls == "pole_window":
        ww, wh = int(rng.integers(1, MAX_WINDOW)), int(rng.integers(1, MAX_WINDOW))
        x0, y0 = -int(rng.integers(0, ww)), -int(rng.integers(0, wh))
        window = (x0, y0, x0 + ww - 1, y0 + wh - 1)
        entry = ("maps", "warp", "fused")[int(rng.integers(0, 3))]
    elif cls == "far_window":
        ww, wh = int(rng.integers(1, MAX_WINDOW)), int(rng.integers(1, MAX_WINDOW))
        mag = float(10.0 ** rng.uniform(2.0, 9.3))
        x0 = int(np.clip(rng.choice([-1, 1]) * mag * rng.uniform(0, 1), -2.0e9, 2.0e9))
        y0 = int(np.clip(rng.choice([-1, 1]) * mag * rng.uniform(0, 1), -2.0e9, 2.0e9))
        window = (x0, y0, x0 + ww - 1, y0 + wh - 1)
        entry = ("maps", "warp", "fused")[int(rng.integers(0, 3))]
    elif cls == "tile_edges" and entry != "roi":
        ww, wh = _edge(rng, COL_BLOCK), _edge(rng, ROW_BLOCK, 12)
        x0, y0 = int(rng.integers(-80, 40)), int(rng.integers(-60, 30))
        window = (x0, y0, x0 + ww - 1, y0 + wh - 1)
    elif cls == "captured":
        entry = ("maps", "warp", "fused")[int(rng.integers(0, 3))]
        if rng.random() < 0.5:          # (else the rig's ROI, found eagerly before the capture, or its window_of)
            ww, wh = _edge(rng, COL_BLOCK), _edge(rng, ROW_BLOCK, 12)
            x0, y0 = int(rng.integers(-80, 40)), int(rng.integers(-60, 30))
            window = (x0, y0, x0 + ww - 1, y0 + wh - 1)
    cn, dtype = TYPES[int(rng.integers(0, len(TYPES)))]
    with_mask = bool(rng.random() < 0.5)
    gain = 1.0 if with_mask or rng.random() < 0.5 else float(rng.uniform(0.4, 2.2))
    return dict(seed=int(seed), cls=cls, kind=kind, rname=rname, w=w, h=h, scale=scale, K=K, R=R, entry=entry, cn=cn, dtype=dtype,
                interp=INTERPS[int(rng.integers(0, len(INTERPS)))], border=BORDERS[int(rng.integers(0, len(BORDERS)))],
                layout="device" if cls == "captured" else LAYOUTS[int(rng.integers(0, len(LAYOUTS)))], window=window, with_mask=with_mask, out16=bool(rng.random() < 0.5), gain=gain,
                img_seed=int(rng.integers(0, 2 ** 31)))


def _place(a, layout, pad=3):
    """The array as the layout's mat: a host array, a device tensor, or a view into a wider host array."""
    if layout == "device":
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if layout == "strided":
        wide = np.zeros((a.shape[0], a.shape[1] + 2 * pad) + a.shape[2:], a.dtype)
        wide[:, pad:pad + a.shape[1]] = a
        return wide[:, pad:pad + a.shape[1]]
    return np.ascontiguousarray(a)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _capture_and_replay(warper, call, overwrite, outs):
    """call() captured once on a side stream (nothing runs), the inputs overwritten and the outputs cleared, then one replay."""
    import gc
    import torch
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    warper.set_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()          # a graph a dead cycle still holds must not be destroyed (a device synchronisation) inside the capture
    with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
        call()
    overwrite()
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()


def run_case(c):
    """Runs the case through the library and the model; returns the list of differences (empty: parity)."""
    import imagestitch_amd as I
    from imagestitch_amd._lib import as_mat, check, f9
    from oracle import capi as O
    m = P.from_rig(c["kind"], c["scale"], c["K"], c["R"])
    warper = I.RotationWarper(c["kind"], c["scale"])
    w, h, K, R = c["w"], c["h"], c["K"], c["R"]
    bad = []
    mroi, mmm = m.detect_roi(w, h)
    mroi = tuple(int(v) for v in mroi)
    if c["window"] is None or c["entry"] == "roi":
        roi, mm = warper.warpRoi((w, h), K, R, with_minmax=True)
        if roi != mroi or not np.array_equal(mm, mmm):
            bad.append("roi %s / %s, model %s / %s" % (roi, mm, mroi, mmm))
        if c["entry"] == "roi":
            return bad
    sane = mroi[2] >= mroi[0] and mroi[3] >= mroi[1] and mroi[2] - mroi[0] < 65536 and mroi[3] - mroi[1] < 65536
    win = c["window"] or (PC.window_of(mroi) if sane else (-61, -50, 66, 45))
    xm, ym = m.build_maps(win)
    captured = c["cls"] == "captured"
    if captured:
        import torch
    if c["entry"] == "maps":
        like = None
        if c["layout"] == "device":
            import torch
            like = torch.empty(1, device="cuda")
        if captured:
            gx, gy = torch.full(xm.shape, 7.0, device="cuda"), torch.full(xm.shape, 7.0, device="cuda")
            mx, my = as_mat(gx), as_mat(gy)
            _capture_and_replay(warper, lambda: check(warper._lib.isx_warper_build_maps_roi(warper._h, f9(K)[1], f9(R)[1], (C.c_int * 4)(*win), C.byref(mx), C.byref(my))),
                                lambda: None, [gx, gy])
        else:
            gx, gy = warper.buildMapsRoi(K, R, win, like=like)
        if not (PC.same_bits(_np(gx), xm) and PC.same_bits(_np(gy), ym)):
            bad.append("maps of %s differ" % (win,))
        return bad
    rng = np.random.default_rng(c["img_seed"])
    if c["entry"] == "warp":
        src = PC.image(rng, h, w, c["cn"], np.dtype(c["dtype"]).type)
        interp, border = c["interp"], c["border"]
        dst = _place(np.zeros(xm.shape + src.shape[2:], src.dtype), c["layout"])
        if captured:
            s, src = _place(src, "device"), PC.image(rng, h, w, c["cn"], np.dtype(c["dtype"]).type)      # the replay reads the second image
            _capture_and_replay(warper, lambda: warper.warp_roi(s, K, R, interp, border, win, dst), lambda: s.copy_(torch.from_numpy(src)), [dst])
            got = _np(dst)
        else:
            got = _np(warper.warp_roi(_place(src, c["layout"]), K, R, interp, border, win, dst))
        want = I.remap(src, xm, ym, interp, border) if (interp & PC.TIES_EVEN or border == PC.WRAP) else O.remap(src, xm, ym, interp, border)
        if not np.array_equal(got, want):
            bad.append("warp of %s differs at %s" % (win, np.argwhere(got != want)[:3].tolist()))
        return bad
    img = PC.image(rng, h, w)
    holes = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
    first = (img, holes)
    if captured:                          # captured on `first`, replayed on these
        img = PC.image(rng, h, w)
        holes = (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
    wi = O.remap(img, xm, ym, PC.LINEAR, PC.REFLECT)
    wm = O.remap(holes if c["with_mask"] else np.full((h, w), 255, np.uint8), xm, ym, PC.NEAREST, PC.CONST)
    if c["gain"] != 1.0:
        wi = PC.gained(wi, c["gain"])
    warper.set_gain(c["gain"])
    di = _place(np.zeros(xm.shape + (3,), np.int16 if c["out16"] else np.uint8), c["layout"])
    dm = _place(np.zeros(xm.shape, np.uint8), c["layout"])
    s, hm = _place(first[0], c["layout"]), (_place(first[1], c["layout"]) if c["with_mask"] else None)
    mi, mdi, mdm = as_mat(s), as_mat(di), as_mat(dm)
    mh = as_mat(hm) if hm is not None else None

    def fused():
        check(warper._lib.isx_warper_warp_with_mask_roi(warper._h, C.byref(mi), C.byref(mh) if mh is not None else None, f9(K)[1], f9(R)[1],
                                                        (C.c_int * 4)(*win), C.byref(mdi), C.byref(mdm)))

    def overwrite():
        s.copy_(torch.from_numpy(img))
        if hm is not None:
            hm.copy_(torch.from_numpy(holes))
    if captured:
        _capture_and_replay(warper, fused, overwrite, [di, dm])
    else:
        fused()
    if not np.array_equal(_np(di), wi.astype(_np(di).dtype)):
        bad.append("fused image of %s differs" % (win,))
    if not np.array_equal(_np(dm), wm):
        bad.append("fused mask of %s differs" % (win,))
    return bad


def run(seconds, seed, verbose=False, progress_path=None):
    """Draws cases (the classes in turn) for `seconds` and compares the library with the model.  Returns a summary dict; progress_path: a file
    that gets the running counts every 30 seconds."""
    import torch
    import imagestitch_amd
    imagestitch_amd.load()
    t0 = time.time()
    per, entries, failing, n, told = {c: 0 for c in CLASSES}, {e: 0 for e in ENTRIES}, [], 0, t0
    while time.time() - t0 < seconds:
        if progress_path and time.time() - told >= 30.0:
            told = time.time()
            with open(progress_path, "w") as f:
                json.dump(dict(seconds=round(told - t0, 1), cases=n, mismatches=len(failing)), f)
        cls = CLASSES[n % len(CLASSES)]
        s = int(seed) * 1000003 + n
        c = case(s, cls)
        bad = run_case(c)
        per[cls] += 1
        entries[c["entry"]] += 1
        n += 1
        if bad:
            failing.append(dict(seed=s, cls=cls, kind=c["kind"], entry=c["entry"], differences=bad[:4]))
            if verbose:
                print("MISMATCH", s, cls, bad[:4], flush=True)
    return dict(tool="fuzz_polar_warp", seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, mismatches=len(failing), per_class=per, per_entry=entries,
                failing_seeds=failing[:20], device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--out", default=None)
    ap.add_argument("--progress", default=None)
    a = ap.parse_args()
    out = run(a.seconds, a.seed, verbose=True, progress_path=a.progress)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(1 if out["mismatches"] else 0)


if __name__ == "__main__":
    main()
