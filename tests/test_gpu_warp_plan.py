"""The decisions of the warper's host code, pinned against a recorded fixture (tests/golden/warp_plan.json).

For a fixed set of cycles on cylindrical, spherical and plane handles - the routing of warp() and warp_with_mask() to their kernels (device
and host mats, pitch-aligned and dense destinations, the gain, a column range), batches (runs of one variant, more than WARP_BATCH_MAX tiles,
a change of variant, a plain warp or a host mat in between, a failing warp), the synchronous detectResultRoi with its two memo lists, planned
warps through every route their verification takes (at once, deferred, batched, discarded and queued again, behind an event, joined), buildMaps
/ buildMapsRoi / remap, and the table arena's start-overs - the fixture holds what the host code decided: per step the launches per launch
name and their summed algorithmic bytes (isx_profile_*), the returned ROIs and corners, table_resets(), and plan_status()'s outcome (OK, or
ISX_ERR_PLAN with its count) for a true plan and for the plan shifted by one pixel in each of its four bounds.  Launches must match exactly;
bytes to a relative 1e-9 - re-associating double additions moves them by about 1e-13, the smallest real accounting change (one pixel's 3
bytes in the smallest tile here) by about 1e-4.  Every image, mask and map produced is also compared bit for bit with the oracle (plane
handles: with the NumPy model tests/helpers/plane_np.py).  Host-side refactors of warp.hip must leave all of it as it is.

    python tests/test_gpu_warp_plan.py --record      # rewrites the fixture from the library as built (on a GPU)
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):      # (run as a script too: --record)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import plan_verify_cases as PC  # noqa: E402
from helpers import plan_verify_np as M  # noqa: E402
from helpers import plane_np as P  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "warp_plan.json")
BYTES_RTOL = 1e-9
CYL, SPH, PLANE = 0, 1, 2
NEAREST, LINEAR = 0, 1
CONST, REFLECT = 0, 2
ERR_PLAN = 8
KIND_NAMES = {CYL: "cyl", SPH: "sph", PLANE: "plane"}
SHIFTS = [(0, -1), (1, -1), (2, 1), (3, 1)]      # one pixel in each of the four bounds (the rectangle grows: every plan can be warped into)


# ---- cameras: (kind, scale, K, R, T, src_w, src_h) ---------------------------------------------------------------------------------------
def _pc(cls, size, kind):
    for c in PC.CASES:
        if c[0] == cls and (c[2], c[3]) == size and c[1] == kind:
            k, scale, K, R, w, h = PC.camera(c)
            return (k, scale, K, R, None, w, h)
    raise KeyError((cls, size, kind))


def _plane(seed, w, h, with_t=True):
    import test_gpu_plane_warp as PW      # its cameras: yaw / pitch / roll up to +-0.5 rad, f of 0.9 .. 2 sides, a translation
    scale, K, R, T = PW._rig(np.random.default_rng(seed), w, h, with_t)
    return (PLANE, scale, K, R, T, w, h)


def _main_cams():
    return {"cyl": _pc("cyl_light", (257, 129), CYL), "sph": _pc("sph_plain", (256, 128), SPH), "plane": _plane(5, 131, 67)}


def _rescaled(cam, scale):
    return (cam[0], scale) + cam[2:]


class _Model:
    """The oracle's ROI of a camera (or a given one), its maps, and cv::remap through them."""

    def __init__(self, oracle, cam, roi=None):
        kind, scale, K, R, T, w, h = cam
        self.oracle = oracle
        if kind == PLANE:
            m = P.from_rig(oracle, scale, K, R, T)
            r = m.detect_roi(w, h)[0] if roi is None else roi
            self.xm, self.ym = m.build_maps(r)
        else:
            k_rinv = oracle.camera(K, R)[3]
            r = oracle.detect_roi(kind, scale, K, R, w, h)[0] if roi is None else roi
            self.xm, self.ym = oracle.build_maps(kind, scale, k_rinv, np.array(r, np.int32))
        self.roi = tuple(int(v) for v in r)
        self.size = (self.roi[2] - self.roi[0] + 1, self.roi[3] - self.roi[1] + 1)

    def warp(self, src, interp=LINEAR, border=REFLECT):
        return self.oracle.remap(src, self.xm, self.ym, interp, border)

    def tile(self, img, mask=None):
        """(warped image, warped mask) of the fused entries: LINEAR / REFLECT and NEAREST / CONSTANT of the all-255 or the caller's mask"""
        return self.warp(img), self.warp(np.full(img.shape[:2], 255, np.uint8) if mask is None else mask, NEAREST, CONST)


def _warper(gpu, cam):
    w = {CYL: gpu.CylindricalWarper, SPH: gpu.SphericalWarper, PLANE: gpu.PlaneWarper}[cam[0]]().create(cam[1])
    if cam[4] is not None:
        w.set_translation(cam[4])
    return w


def _src(cam, seed, cn=3, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (cam[6], cam[5], cn) if cn > 1 else (cam[6], cam[5])).astype(np.uint8)
    return a if dtype == np.uint8 else a.astype(np.float32) * np.float32(1.37)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _put(a, device):
    import torch
    return torch.from_numpy(a).cuda() if device else a


def _dsts(size, out16=False, device=True, pitched=False, fill=None):
    """(dst_img, dst_mask) of a warped tile: dense, or with rows pitched to 64 bytes (device only)"""
    import torch
    dw, dh = size
    dt, es = (torch.int16, 2) if out16 else (torch.uint8, 1)
    if not device:
        return np.full((dh, dw, 3), fill or 0, np.int16 if out16 else np.uint8), np.full((dh, dw), fill or 0, np.uint8)
    if not pitched:
        di, dm = torch.zeros((dh, dw, 3), dtype=dt, device="cuda"), torch.zeros((dh, dw), dtype=torch.uint8, device="cuda")
    else:
        pi, pm = (dw * 3 * es + 63) // 64 * 64, (dw + 63) // 64 * 64
        di = torch.zeros(dh * pi // es, dtype=dt, device="cuda").as_strided((dh, dw, 3), (pi // es, 3, 1))
        dm = torch.zeros(dh * pm, dtype=torch.uint8, device="cuda").as_strided((dh, dw), (pm, 1))
    if fill is not None:
        di.fill_(fill); dm.fill_(fill)
    return di, dm


def _same(got, want, what):
    got = _np(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])


# ---- recording ---------------------------------------------------------------------------------------------------------------------------
class _Profile:
    """with _Profile() as p: ...; p.launches = {launch name: [launches, algorithmic bytes]} of the calls inside."""

    def __enter__(self):
        from imagestitch_amd import _lib
        lib = _lib.load()
        lib.isx_profile_enable(1); lib.isx_profile_filter(None); lib.isx_profile_sample(1); lib.isx_profile_reset()
        self.launches = None
        return self

    def __exit__(self, *exc):
        from imagestitch_amd import _lib
        try:
            if exc[0] is None:
                self.launches = {k: [int(v["launches"]), float(v["alg_bytes"])] for k, v in sorted(_lib.profile_entries().items())}
        finally:
            _lib.load().isx_profile_enable(0)
        return False


class _Rec:
    """What one cycle records: the launch table of each named step, and whatever else the cycle notes (ROIs, corners, statuses, errors)."""

    def __init__(self):
        self.steps, self.notes = [], {}

    def step(self, name, fn):
        with _Profile() as p:
            out = fn()
        self.steps.append([name, p.launches])
        return out

    def note(self, key, value):
        self.notes.setdefault(key, []).append(value)

    def refused(self, gpu, name, fn):
        """a step that must fail: its code and message are noted, and what it launched before failing"""
        def run():
            with pytest.raises(gpu.IsxError) as e:
                fn()
            return [int(e.value.code), str(e.value)]
        self.note("errors", [name] + self.step(name, run))

    def done(self, warper=None):
        if warper is not None:
            self.notes["table_resets"] = int(warper.table_resets())
        return {"steps": self.steps, "notes": self.notes}


def _status(w):
    """isx_warper_plan_status -> [return code, *mismatches]"""
    n = C.c_int(-1)
    rc = w._lib.isx_warper_plan_status(w._h, C.byref(n))
    assert rc in (0, ERR_PLAN) and (rc == 0) == (n.value == 0), (rc, n.value)
    return [int(rc), int(n.value)]


# ---- cycle 1: warp() ----------------------------------------------------------------------------------------------------------------------
WARP_ROUTES = [("u8c3-linear-reflect", 3, np.uint8, LINEAR, REFLECT), ("u8c1-nearest-constant", 1, np.uint8, NEAREST, CONST),
               ("u8c3-nearest-reflect", 3, np.uint8, NEAREST, REFLECT), ("u8c1-linear-reflect", 1, np.uint8, LINEAR, REFLECT),
               ("f32c1-linear-reflect", 1, np.float32, LINEAR, REFLECT), ("f32c3-linear-reflect", 3, np.float32, LINEAR, REFLECT)]


def _warp_routing(gpu, oracle, cam, device):
    rec, m, w = _Rec(), _Model(oracle, cam), _warper(gpu, cam)
    for j, (name, cn, dtype, interp, border) in enumerate(WARP_ROUTES):
        src = _src(cam, 100 + j, cn, dtype)
        corner, dst = rec.step(name, lambda: w.warp(_put(src, device), cam[2], cam[3], interp, border))      # isx_warper_roi + isx_warper_warp_roi
        rec.note("corners", list(corner))
        _same(dst, m.warp(src, interp, border), name)
    src = _src(cam, 99)
    dst = _put(np.zeros(m.size[::-1] + (3,), np.uint8), device)
    corner, dst = rec.step("own-roi", lambda: w.warp(_put(src, device), cam[2], cam[3], LINEAR, REFLECT, dst=dst))      # isx_warper_warp
    rec.note("corners", list(corner))
    _same(dst, m.warp(src), "own-roi")
    return rec.done(w)


# ---- cycle 2: warp_with_mask() ------------------------------------------------------------------------------------------------------------
def _mask_routing(gpu, oracle, cam, variant):
    rec, m, w = _Rec(), _Model(oracle, cam), _warper(gpu, cam)
    K, R = cam[2], cam[3]
    dw, dh = m.size
    assert dw % 4 != 0 and dw > 80, m.size      # dense rows are not whole dwords; the column range below starts in the second 64-column block
    img = _src(cam, 200)
    holes = (np.random.default_rng(201).integers(0, 4, img.shape[:2]) > 0).astype(np.uint8) * 255
    wi, wm = m.tile(img)
    _, wh = m.tile(img, holes)
    lo, hi = 0, dw
    if variant == "gain":
        w.set_gain(1.25)
        wi = oracle.gain_apply(wi, 1.25)
    if variant == "columns":
        w.set_dst_columns(70, dw - 7)
        lo, hi = 64, dw - 7
    for device in (True, False):
        how = "dev" if device else "host"
        for out16 in (False, True):
            name = "nomask-%s-%s" % ("16s" if out16 else "8u", how)
            di, dm = _dsts(m.size, out16, device, fill=77)
            corner, gi, gm = rec.step(name, lambda: w.warp_with_mask(_put(img, device), K, R, dst_img=di, dst_mask=dm))
            rec.note("corners", list(corner))
            gi, gm, want = _np(gi), _np(gm), wi.astype(np.int16 if out16 else np.uint8)
            _same(gi[:, lo:hi], want[:, lo:hi], name); _same(gm[:, lo:hi], wm[:, lo:hi], name)
            assert (gi[:, :lo] == 77).all() and (gi[:, hi:] == 77).all() and (gm[:, :lo] == 77).all() and (gm[:, hi:] == 77).all(), name
    if variant == "gain":      # the gain goes with the all-255 mask only
        di, dm = _dsts(m.size)
        rec.refused(gpu, "gain-with-mask", lambda: w.warp_with_mask(_put(img, True), K, R, mask=_put(holes, True), dst_img=di, dst_mask=dm))
        w.set_gain(1.0)
    for pitched in (True, False):      # a caller's mask: k_warp_img_mask, dword stores for aligned rows (a column range does not apply)
        for out16 in (False, True):
            name = "mask-%s-%s" % ("16s" if out16 else "8u", "pitched" if pitched else "dense")
            di, dm = _dsts(m.size, out16, True, pitched)
            corner, gi, gm = rec.step(name, lambda: w.warp_with_mask(_put(img, True), K, R, mask=_put(holes, True), dst_img=di, dst_mask=dm))
            _same(gi, m.warp(img).astype(np.int16 if out16 else np.uint8), name); _same(gm, wh, name)
    return rec.done(w)


# ---- cycle 3: batches ---------------------------------------------------------------------------------------------------------------------
def _batches(gpu, oracle, cam):
    rec, m, w = _Rec(), _Model(oracle, cam), _warper(gpu, cam)
    K, R = cam[2], cam[3]
    img = _src(cam, 300)
    gray = _src(cam, 301, 1)
    wi, wm = m.tile(img)
    dimg = _put(img, True)
    made = []

    def tile(out16=False, device=True):
        di, dm = _dsts(m.size, out16, device)
        corner, gi, gm = w.warp_with_mask(dimg if device else img, K, R, dst_img=di, dst_mask=dm)
        assert corner == m.roi[:2]
        made.append((gi, gm, out16))

    def batch(name, fn):
        def run():
            w.begin_batch()
            fn()
            w.end_batch()
        rec.step(name, run)

    batch("3-of-one-variant", lambda: [tile() for _ in range(3)])
    batch("9-of-one-variant", lambda: [tile() for _ in range(9)])
    batch("8u-16s-16s-8u", lambda: [tile(o) for o in (False, True, True, False)])

    def with_plain():
        tile(); tile()
        _, g = w.warp(_put(gray, True), K, R, NEAREST, CONST, dst=_put(np.zeros(m.size[::-1], np.uint8), True))
        _same(g, m.warp(gray, NEAREST, CONST), "plain warp inside a batch")
        tile()
    batch("plain-warp-in-the-middle", with_plain)
    batch("host-mat-in-the-middle", lambda: [tile(device=d) for d in (True, False, True)])

    def failing():
        w.begin_batch()
        tile(); tile()
        di, dm = _dsts((m.size[0] + 1, m.size[1]))
        w.warp_with_mask(dimg, K, R, dst_img=di, dst_mask=dm)      # ISX_ERR_SIZE: ends the batch, the two collected tiles leave
    rec.refused(gpu, "failing-warp", failing)
    rec.step("after-the-failure", lambda: tile())                  # not batching any more: launched at once
    batch("next-batch-is-empty", lambda: None)
    for gi, gm, out16 in made:
        _same(gi, wi.astype(np.int16) if out16 else wi, "batched tile"); _same(gm, wm, "batched mask")
    return rec.done(w)


# ---- cycle 4: the synchronous detectResultRoi ---------------------------------------------------------------------------------------------
ROI_CAMS = {"cyl_light": lambda: _pc("cyl_light", (257, 129), CYL), "cyl_light_700": lambda: _pc("cyl_light", (700, 500), CYL),
            "cyl_pole": lambda: _pc("cyl_pole", (33, 33), CYL), "cyl_corner_behind": lambda: _pc("cyl_corner_behind", (256, 128), CYL),
            "sph_plain": lambda: _pc("sph_plain", (256, 128), SPH), "sph_north": lambda: _pc("sph_north", (257, 129), SPH),
            "sph_south": lambda: _pc("sph_south", (33, 33), SPH), "plane": lambda: _plane(5, 131, 67), "plane_no_t": lambda: _plane(4, 33, 33, False)}


def _ask_roi(rec, w, cam, name, want):
    roi, mm = rec.step(name, lambda: w.warpRoi((cam[5], cam[6]), cam[2], cam[3], with_minmax=True))
    rec.note("rois", [list(roi), [float(v) for v in mm]])
    assert tuple(roi) == want, (name, roi, want)


def _roi_twice(gpu, oracle, cam):
    rec, m, w = _Rec(), _Model(oracle, cam), _warper(gpu, cam)
    _ask_roi(rec, w, cam, "first", m.roi)
    _ask_roi(rec, w, cam, "second", m.roi)
    return rec.done(w)


def _roi_alternate(gpu, oracle):
    """two cylindrical full-scan cameras A and B on one handle (one scale), asked for A B A B: without set_roi_cache only the last result is
    kept (four scans), with it both are (two scans); switching it off again clears the list (B, the last one asked for, is scanned again)"""
    a = _pc("cyl_pole", (33, 33), CYL)
    b = _rescaled(_pc("cyl_corner_behind", (129, 46), CYL), a[1])
    rec = _Rec()
    want = {id(a): _Model(oracle, a).roi, id(b): _Model(oracle, b).roi}
    for phase in ("off", "on"):
        w = _warper(gpu, a)
        w.set_roi_cache(phase == "on")
        for j, cam in enumerate((a, b, a, b)):
            _ask_roi(rec, w, cam, "%s-%s%d" % (phase, "ab"[j % 2], j // 2), want[id(cam)])
    w.set_roi_cache(False)
    _ask_roi(rec, w, b, "off-again-b0", want[id(b)])
    _ask_roi(rec, w, b, "off-again-b1", want[id(b)])
    return rec.done(w)


# ---- cycle 5: planned warps ---------------------------------------------------------------------------------------------------------------
PLAN_CAMS = {"cyl_light": lambda: _pc("cyl_light", (257, 129), CYL), "cyl_pole": lambda: _pc("cyl_pole", (33, 33), CYL),
             "cyl_corner_behind": lambda: _pc("cyl_corner_behind", (129, 46), CYL), "sph_plain": lambda: _pc("sph_plain", (256, 128), SPH),
             "sph_north": lambda: _pc("sph_north", (33, 33), SPH), "sph_south": lambda: _pc("sph_south", (33, 33), SPH),
             "plane": lambda: _plane(5, 131, 67)}
PLAN_ROUTES = ["immediate", "deferred", "batch", "discard-queue-verify", "verify-after", "join"]


def _planned(gpu, oracle, cam, route):
    import torch
    rec, w = _Rec(), _warper(gpu, cam)
    K, R, size = cam[2], cam[3], (cam[5], cam[6])
    true = _Model(oracle, cam).roi
    img = _src(cam, 500)
    dimg = _put(img, True)
    keep = []
    for shift in [None] + SHIFTS:
        plan = true if shift is None else tuple(M.shifted(list(true), *shift))
        tag = "true" if shift is None else "bound%d%+d" % shift
        m = _Model(oracle, cam, plan)
        di, dm = _dsts(m.size)

        def warp():
            w.warp_with_mask_planned(dimg, K, R, plan, di, dm)
        if route == "immediate":
            rec.step(tag, warp)
        elif route == "deferred":
            w.set_deferred_verify(True)
            rec.step(tag + "-warp", warp)
            rec.step(tag + "-verify", w.verify)
            w.set_deferred_verify(False)
        elif route == "batch":
            w.begin_batch()
            rec.step(tag + "-collect", warp)
            rec.step(tag + "-end", w.end_batch)
        elif route == "discard-queue-verify":
            w.set_deferred_verify(True)
            rec.step(tag + "-warp", warp)
            w.discard_pending()
            rec.step(tag + "-verify-nothing", w.verify)
            rec.step(tag + "-queue", lambda: w.queue_verify(size, K, R, plan))
            rec.step(tag + "-verify", w.verify)
            w.set_deferred_verify(False)
        elif route == "verify-after":
            ev = torch.cuda.Event()
            ev.record()
            keep.append(ev)
            w.queue_verify(size, K, R, plan)
            rec.step(tag, lambda: w.verify_after(ev))
        else:
            def joined():
                warp()
                w.join()
            rec.step(tag, joined)
        rec.note("plan_status", [tag] + _status(w))
        if route != "verify-after":
            wi, wm = m.tile(img)
            _same(di, wi, (route, tag)); _same(dm, wm, (route, tag))
    torch.cuda.synchronize()
    return rec.done(w)


def _planned_border_three_passes(gpu, oracle):
    """700 x 500: the one-workgroup border scan walks its 2400 border pixels in three passes of 1024 threads"""
    cam = _pc("cyl_light", (700, 500), CYL)
    rec, w = _Rec(), _warper(gpu, cam)
    true = _Model(oracle, cam).roi
    for shift in [None] + SHIFTS:
        plan = true if shift is None else tuple(M.shifted(list(true), *shift))
        tag = "true" if shift is None else "bound%d%+d" % shift
        w.queue_verify((700, 500), cam[2], cam[3], plan)
        rec.step(tag, w.verify)
        rec.note("plan_status", [tag] + _status(w))
    return rec.done(w)


# ---- cycle 6: buildMaps / buildMapsRoi / remap --------------------------------------------------------------------------------------------
def _maps(gpu, oracle, cam):
    import torch
    rec, m, w = _Rec(), _Model(oracle, cam), _warper(gpu, cam)
    like = torch.empty(1, device="cuda")
    for how, lk in (("host", None), ("dev", like)):
        roi, xm, ym = rec.step("buildMaps-" + how, lambda: w.buildMaps((cam[5], cam[6]), cam[2], cam[3], like=lk))
        rec.note("rois", list(roi))
        assert tuple(roi) == m.roi
        _same(xm, m.xm, "xmap"); _same(ym, m.ym, "ymap")
        part = (m.roi[0] + 3, m.roi[1] - 2, m.roi[0] + 3 + 70, m.roi[1] + 9)      # a rectangle of its own: 71 x 12
        xm, ym = rec.step("buildMapsRoi-" + how, lambda: w.buildMapsRoi(cam[2], cam[3], part, like=lk))
        mp = _Model(oracle, cam, part)
        _same(xm, mp.xm, "xmap of a given rectangle"); _same(ym, mp.ym, "ymap of a given rectangle")
    return rec.done(w)


def _remap(gpu, oracle):
    cam = _main_cams()["cyl"]
    rec, m = _Rec(), _Model(oracle, cam)
    for cn, dtype, tn in ((1, np.uint8, "u8c1"), (3, np.uint8, "u8c3"), (1, np.float32, "f32c1"), (3, np.float32, "f32c3")):
        src = _src(cam, 600 + cn, cn, dtype)
        for interp, border, ib in ((NEAREST, CONST, "nearest-constant"), (LINEAR, REFLECT, "linear-reflect")):
            for device in (True, False):
                name = "%s-%s-%s" % (tn, ib, "dev" if device else "host")
                dst = rec.step(name, lambda: gpu.remap(_put(src, device), _put(m.xm, device), _put(m.ym, device), interp, border))
                _same(dst, m.warp(src, interp, border), name)
    return rec.done()


# ---- cycle 7: the table arena, counts only ------------------------------------------------------------------------------------------------
def _arena(gpu, oracle, cam):
    import torch
    from imagestitch_amd._lib import as_mat, check, f9
    rec, w = _Rec(), _warper(gpu, cam)
    _k, kp = f9(cam[2])
    _r, rp = f9(cam[3])
    xm, ym = torch.empty((8, 8), dtype=torch.float32, device="cuda"), torch.empty((8, 8), dtype=torch.float32, device="cuda")
    mx, my = as_mat(xm), as_mat(ym)

    def maps(i):
        check(w._lib.isx_warper_build_maps_roi(w._h, kp, rp, (C.c_int * 4)(i, 5, i + 7, 12), C.byref(mx), C.byref(my)))
    rec.step("same-roi-twice", lambda: [maps(0), maps(0)])
    rec.note("resets_after", int(w.table_resets()))
    for i in range(1, 2100):      # 1024 entries: the 1025th and the 2049th distinct rectangle start the arena over
        maps(i)
        if i in (1023, 1024, 1100, 2047, 2048, 2099):
            rec.note("resets_after", int(w.table_resets()))
    mp = _Model(oracle, cam, (2099, 5, 2106, 12))
    _same(xm, mp.xm, "xmap after two start-overs"); _same(ym, mp.ym, "ymap after two start-overs")
    rec.step("an-old-roi-again", lambda: maps(0))
    _same(xm, _Model(oracle, cam, (0, 5, 7, 12)).xm, "xmap of a rectangle dropped by a start-over")
    return rec.done(w)


def _cases():
    c = {}
    for kn, cam in _main_cams().items():
        for device in (True, False):
            c["warp-%s-%s" % (kn, "dev" if device else "host")] = lambda g, o, cam=cam, device=device: _warp_routing(g, o, cam, device)
        for variant in ("plain", "gain", "columns"):
            c["mask-%s-%s" % (kn, variant)] = lambda g, o, cam=cam, variant=variant: _mask_routing(g, o, cam, variant)
        c["batch-%s" % kn] = lambda g, o, cam=cam: _batches(g, o, cam)
        c["maps-%s" % kn] = lambda g, o, cam=cam: _maps(g, o, cam)
        c["arena-%s" % kn] = lambda g, o, cam=cam: _arena(g, o, cam)
    for name, mk in ROI_CAMS.items():
        c["roi-twice-%s" % name] = lambda g, o, mk=mk: _roi_twice(g, o, mk())
    c["roi-alternate"] = _roi_alternate
    for name, mk in PLAN_CAMS.items():
        for route in PLAN_ROUTES:
            c["planned-%s-%s" % (name, route)] = lambda g, o, mk=mk, route=route: _planned(g, o, mk(), route)
    c["planned-cyl_light_700-border-three-passes"] = _planned_border_three_passes
    c["remap"] = _remap
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_decisions_equal_the_recorded_ones(gpu, oracle, golden, case):
    got, want = json.loads(json.dumps(CASES[case](gpu, oracle))), golden[case]
    print(case, json.dumps(got, sort_keys=True))
    assert got["notes"] == want["notes"], (case, got["notes"], want["notes"])
    assert [s[0] for s in got["steps"]] == [s[0] for s in want["steps"]], case
    for (step, launches), (_step, wlaunches) in zip(got["steps"], want["steps"]):
        assert sorted(launches) == sorted(wlaunches), (case, step, sorted(launches), sorted(wlaunches))
        for name, (n, by) in launches.items():
            wn, wby = wlaunches[name]
            assert n == wn, (case, step, name, n, wn)
            assert abs(by - wby) <= BYTES_RTOL * abs(wby), (case, step, name, by, wby)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_warp_plan.py --record")
    import imagestitch_amd
    from oracle import capi
    imagestitch_amd.load()
    capi.lib()
    out = {}
    for case_id in sorted(CASES):
        out[case_id] = CASES[case_id](imagestitch_amd, capi)
        print(case_id, flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases in %s" % (len(out), GOLDEN))
