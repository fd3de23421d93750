"""Long-lived fisheye and stereographic handles (tests/test_gpu_handle_lifetime.py covers the tabulated kinds): what one handle carries from
call to call, against the NumPy model tests/helpers/polar_np.py bit for bit.

- one hipGraph that holds buildMaps, two warps and two fused warps of one handle: replayed, replayed over new source bytes, replayed after
  eager calls of the same handle with another camera, window and gain, replayed after the handle moved to another stream;
- the capture rule (the polar section, "Capture"): a self-ROI entry whose ROI is not remembered and every entry with a host mat
  are ISX_ERR_STATE on a capturing stream, before anything is enqueued and before the handle changes; a remembered ROI is served;
- four threads, two handles of each kind, every call's ROI scan on the one ROI stream all handles of a device share;
- the ROI memo past its 1024 entries, revisited, switched off, and keyed by the source size.

Expected pixels: oracle.remap over the MODEL's maps; np.array_equal / same_bits, no tolerance."""
import ctypes as C
import gc
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polar_cases as PC  # noqa: E402
from helpers import polar_np as P  # noqa: E402

from imagestitch_amd._lib import as_mat, check, f9  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = [P.FISHEYE, P.STEREOGRAPHIC]
ERR_STATE = 3


def _warper(gpu, kind, scale):
    return (gpu.FisheyeWarper if kind == P.FISHEYE else gpu.StereographicWarper)().create(scale)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _window(roi, origin=False):
    """At most 128 x 96 of the rig's ROI, from its top-left corner; origin: the window of a blown-up rig around the destination origin."""
    if origin:
        return (-61, -50, 66, 45)
    roi = tuple(int(v) for v in roi)
    return (roi[0], roi[1], min(roi[2], roi[0] + 127), min(roi[3], roi[1] + 95))


def _shape(win):
    return (win[3] - win[1] + 1, win[2] - win[0] + 1)


def _maps_roi(warper, K, R, win, xm, ym):
    mx, my = as_mat(xm), as_mat(ym)
    check(warper._lib.isx_warper_build_maps_roi(warper._h, f9(K)[1], f9(R)[1], (C.c_int * 4)(*[int(v) for v in win]), C.byref(mx), C.byref(my)))


def _maps_self(warper, w, h, K, R, xm, ym):
    mx, my = as_mat(xm), as_mat(ym)
    check(warper._lib.isx_warper_build_maps(warper._h, int(w), int(h), f9(K)[1], f9(R)[1], C.byref(mx), C.byref(my), (C.c_int * 4)()))


def _fused_roi(warper, img, mask, K, R, win, dimg, dmask):
    mi, mdi, mdm = as_mat(img), as_mat(dimg), as_mat(dmask)
    mm = as_mat(mask) if mask is not None else None
    check(warper._lib.isx_warper_warp_with_mask_roi(warper._h, C.byref(mi), C.byref(mm) if mm is not None else None, f9(K)[1], f9(R)[1],
                                                    (C.c_int * 4)(*[int(v) for v in win]), C.byref(mdi), C.byref(mdm)))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _zeros(shape, dt, fill=0):
    import torch
    return torch.full(tuple(shape), fill, dtype=getattr(torch, np.dtype(dt).name), device="cuda")


class _Step:
    """The five calls of the captured step on one camera, two windows and one gain, and what the model says they write."""

    def __init__(self, kind, f, K, R, win, win2, gain):
        self.kind, self.f, self.K, self.R, self.win, self.win2, self.gain = kind, f, K, R, win, win2, gain
        m = P.from_rig(kind, f, K, R)
        self.xm, self.ym = m.build_maps(win)
        self.xm2, self.ym2 = m.build_maps(win2)
        s, s2 = _shape(win), _shape(win2)
        self.out = dict(xm=_zeros(s, F), ym=_zeros(s, F), w8=_zeros(s + (3,), np.uint8), wf=_zeros(s2, F), di=_zeros(s + (3,), np.uint8), dm=_zeros(s, np.uint8),
                        d16=_zeros(s + (3,), np.int16), dm16=_zeros(s, np.uint8))

    def issue(self, warper, src8, srcf, mask):
        o = self.out
        _maps_roi(warper, self.K, self.R, self.win, o["xm"], o["ym"])
        warper.warp_roi(src8, self.K, self.R, PC.LINEAR, PC.REFLECT, self.win, o["w8"])
        warper.warp_roi(srcf, self.K, self.R, PC.NEAREST, PC.CONST, self.win2, o["wf"])
        warper.set_gain(1.0)
        _fused_roi(warper, src8, mask, self.K, self.R, self.win, o["di"], o["dm"])
        warper.set_gain(self.gain)
        _fused_roi(warper, src8, None, self.K, self.R, self.win, o["d16"], o["dm16"])

    def clear(self):
        for t in self.out.values():
            t.zero_()

    def check(self, oracle, src8, srcf, mask, what):
        o = {k: v.cpu().numpy() for k, v in self.out.items()}
        w8 = oracle.remap(src8, self.xm, self.ym, PC.LINEAR, PC.REFLECT)
        assert PC.same_bits(o["xm"], self.xm) and PC.same_bits(o["ym"], self.ym), what
        assert np.array_equal(o["w8"], w8), (what, "warp 8UC3")
        assert np.array_equal(o["wf"], oracle.remap(srcf, self.xm2, self.ym2, PC.NEAREST, PC.CONST)), (what, "warp 32FC1")
        assert np.array_equal(o["di"], w8) and np.array_equal(o["dm"], oracle.remap(mask, self.xm, self.ym, PC.NEAREST, PC.CONST)), (what, "fused with a mask")
        assert np.array_equal(o["d16"], PC.gained(w8, self.gain).astype(np.int16)), (what, "fused 16SC3 with the gain")
        assert np.array_equal(o["dm16"], oracle.remap(np.full(mask.shape, 255, np.uint8), self.xm, self.ym, PC.NEAREST, PC.CONST)), (what, "fused all-255 mask")


def _sources(rng, h, w):
    return PC.image(rng, h, w), PC.image(rng, h, w, 1, np.float32), (rng.integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255


# ---- a. one graph, three entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_graph_of_maps_warps_and_fused_warps(gpu, oracle, kind):
    """build_maps_roi, warp_roi and warp_with_mask_roi on device mats are one kernel each, the camera and the gain table in its arguments:
    a graph of them replays the captured camera, windows and gain whatever the handle served in between and wherever it moved."""
    import torch
    w, h, f, K, R = P.rig(P.SIZES[0], "yaw0.52")
    warper = _warper(gpu, kind, f)
    roi = warper.warpRoi((w, h), K, R)
    assert roi == tuple(int(v) for v in P.from_rig(kind, f, K, R).detect_roi(w, h)[0])
    rng = np.random.default_rng(70 + kind)
    src8, srcf, mask = _sources(rng, h, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    warper.set_stream(s)
    with torch.cuda.stream(s):
        step = _Step(kind, f, K, R, _window(roi), _window(roi, origin=True), 1.37)
        d8, df, dmask = _dev(src8), _dev(srcf), _dev(mask)
        # the eager calls in between: the other rig's source size and camera (at the handle's scale), other windows, another gain
        w2, h2, _, K2, R2 = P.rig(P.SIZES[1], "pitch-pi/3")
        eager = _Step(kind, f, K2, R2, (5, -40, 90, 30), (-20, -30, 80, 40), 0.5)
        e8, ef, emask = _sources(rng, h2, w2)
        de8, def_, demask = _dev(e8), _dev(ef), _dev(emask)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()                                              # (see test_table_miss_while_capturing_is_refused)
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        step.issue(warper, d8, df, dmask)
    torch.cuda.synchronize()
    assert all(int(t.abs().sum()) == 0 for t in step.out.values()), "a captured call ran"
    g.replay()
    torch.cuda.synchronize()
    step.check(oracle, src8, srcf, mask, "replay")
    # new source bytes in the same tensors
    src8, srcf, mask = _sources(rng, h, w)
    d8.copy_(torch.from_numpy(src8)); df.copy_(torch.from_numpy(srcf)); dmask.copy_(torch.from_numpy(mask))
    step.clear()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    step.check(oracle, src8, srcf, mask, "replay over new source bytes")
    # eager calls of the same handle: another camera, other windows, another gain (left set on the handle)
    with torch.cuda.stream(s):
        eager.issue(warper, de8, def_, demask)
    s.synchronize()
    eager.check(oracle, e8, ef, emask, "eager between replays")
    step.clear()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    step.check(oracle, src8, srcf, mask, "replay after eager calls with another camera")
    # the handle moves to another stream; the graph replays where it is launched
    s2 = torch.cuda.Stream()
    warper.set_stream(s2)
    with torch.cuda.stream(s2):
        eager.clear()
        eager.issue(warper, de8, def_, demask)
    s2.synchronize()
    eager.check(oracle, e8, ef, emask, "eager on the new stream")
    step.clear()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    step.check(oracle, src8, srcf, mask, "replay after set_stream")


# ---- b. the capture rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_capture_rule(gpu, oracle, kind):
    """On a capturing stream: detectResultRoi of a camera the memo does not hold (it allocates, copies on the ROI stream and synchronises)
    and any host mat (staged through an allocation, a copy and a synchronisation) are ISX_ERR_STATE with a message that says why - nothing
    enqueued, the capture intact, no destination touched, the handle's memo as it was: the remembered camera is served into the same
    capture AFTER the refusals.  Relaxed capture mode: a missing refusal fails pytest.raises and nothing else."""
    import torch
    w, h, f, KA, RA = P.rig(P.SIZES[0], "yaw0.52")
    _, _, _, KB, RB = P.rig(P.SIZES[0], "identity")
    mA = P.from_rig(kind, f, KA, RA)
    roiA = tuple(int(v) for v in mA.detect_roi(w, h)[0])
    xmA, ymA = mA.build_maps(roiA)
    src = PC.image(np.random.default_rng(11 + kind), h, w)
    holes = (np.random.default_rng(12).integers(0, 4, (h, w)) > 0).astype(np.uint8) * 255
    wantA = oracle.remap(src, xmA, ymA, PC.LINEAR, PC.REFLECT)
    wantMaskA = oracle.remap(np.full((h, w), 255, np.uint8), xmA, ymA, PC.NEAREST, PC.CONST)
    warper = _warper(gpu, kind, f)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    warper.set_stream(s)
    shp = _shape(roiA)
    with torch.cuda.stream(s):
        dsrc, dholes = _dev(src), _dev(holes)
        x = torch.zeros(16, device="cuda")
        # every destination starts as 7s; `hit*` are the served calls' own
        dev = {k: _zeros(shp + (3,), np.uint8, 7) for k in ("warp", "fused_img", "roi_img", "hit", "hit_img")}
        dev.update({k: _zeros(shp, np.uint8, 7) for k in ("fused_mask", "roi_mask", "hit_mask")})
        dev.update({k: _zeros(shp, F, 7) for k in ("xm", "ym", "hit_xm", "hit_ym")})
        assert warper.warpRoi((w, h), KA, RA) == roiA                      # the one query before capture: the memo holds camera A
    host = dict(img=np.full(shp + (3,), 7, np.uint8), mask=np.full(shp, 7, np.uint8), xm=np.full(shp, 7, F), ym=np.full(shp, 7, F))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()                                              # (see test_table_miss_while_capturing_is_refused)

    def refused(call, why):
        with pytest.raises(gpu.IsxError) as e:
            call()
        assert e.value.code == ERR_STATE and "capturing" in e.value.msg and why in e.value.msg, e.value.msg
        del e

    miss, staged = "query the ROI once before capture", "host mat"
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        # the entries that find the ROI themselves, camera B: not remembered
        refused(lambda: warper.warpRoi((w, h), KB, RB), miss)
        refused(lambda: warper.warp(dsrc, KB, RB, PC.LINEAR, PC.REFLECT, dst=dev["warp"]), miss)
        refused(lambda: warper.warp_with_mask(dsrc, KB, RB, dst_img=dev["fused_img"], dst_mask=dev["fused_mask"]), miss)
        refused(lambda: _maps_self(warper, w, h, KB, RB, dev["xm"], dev["ym"]), miss)
        refused(lambda: warper.warpRoi((w + 1, h), KA, RA), miss)          # camera A at another source size: the size is part of the key
        # a host mat in each position, the ROI given (camera A)
        refused(lambda: warper.warp_roi(src, KA, RA, PC.LINEAR, PC.REFLECT, roiA, dev["warp"]), staged)
        refused(lambda: warper.warp_roi(dsrc, KA, RA, PC.LINEAR, PC.REFLECT, roiA, host["img"]), staged)
        refused(lambda: _fused_roi(warper, src, None, KA, RA, roiA, dev["roi_img"], dev["roi_mask"]), staged)
        refused(lambda: _fused_roi(warper, dsrc, holes, KA, RA, roiA, dev["roi_img"], dev["roi_mask"]), staged)
        refused(lambda: _fused_roi(warper, dsrc, None, KA, RA, roiA, host["img"], dev["roi_mask"]), staged)
        refused(lambda: _fused_roi(warper, dsrc, None, KA, RA, roiA, dev["roi_img"], host["mask"]), staged)
        refused(lambda: _maps_roi(warper, KA, RA, roiA, host["xm"], dev["ym"]), staged)
        refused(lambda: _maps_roi(warper, KA, RA, roiA, dev["xm"], host["ym"]), staged)
        refused(lambda: warper.warp(src, KA, RA, PC.LINEAR, PC.REFLECT, dst=dev["warp"]), staged)      # remembered ROI, host source
        # camera A is still the remembered one: the same entries are served into this capture
        assert warper.warpRoi((w, h), KA, RA) == roiA
        assert warper.warp(dsrc, KA, RA, PC.LINEAR, PC.REFLECT, dst=dev["hit"])[0] == roiA[:2]
        assert warper.warp_with_mask(dsrc, KA, RA, dst_img=dev["hit_img"], dst_mask=dev["hit_mask"])[0] == roiA[:2]
        _maps_self(warper, w, h, KA, RA, dev["hit_xm"], dev["hit_ym"])
    torch.cuda.synchronize()
    assert float(x[0]) == 0.0 and all(bool((t == 7).all()) for t in dev.values()), "something ran or was written during the capture"
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    for k, t in dev.items():
        if not k.startswith("hit"):
            assert bool((t == 7).all()), k
    assert all((a == 7).all() for a in host.values())
    assert np.array_equal(_np(dev["hit"]), wantA) and np.array_equal(_np(dev["hit_img"]), wantA) and np.array_equal(_np(dev["hit_mask"]), wantMaskA)
    assert PC.same_bits(_np(dev["hit_xm"]), xmA) and PC.same_bits(_np(dev["hit_ym"]), ymA)
    # the handle afterwards: both cameras eagerly, host and device mats
    with torch.cuda.stream(s):
        c, got = warper.warp(dsrc, KA, RA, PC.LINEAR, PC.REFLECT, dst=dev["warp"])
        assert c == roiA[:2] and np.array_equal(_np(got), wantA)
        mB = P.from_rig(kind, f, KB, RB)
        roiB = tuple(int(v) for v in mB.detect_roi(w, h)[0])
        assert warper.warpRoi((w, h), KB, RB) == roiB
        xmB, ymB = mB.build_maps(roiB)
        c, got = warper.warp(src, KB, RB, PC.LINEAR, PC.REFLECT)
        assert c == roiB[:2] and np.array_equal(got, oracle.remap(src, xmB, ymB, PC.LINEAR, PC.REFLECT))


# ---- c. four threads ----------------------------------------------------------------------------------------------------------------------------
def test_four_threads_share_the_roi_stream(gpu, oracle):
    """Four handles, two of each kind, each in its own thread on its own stream: warpRoi with the cache off (every call scans on the one ROI
    stream the handles of a device share, each with its own keys and pinned landing zone), buildMapsRoi, warp_roi and warp_with_mask;
    everything is kept and compared with the model after the join.  isx_last_error stays empty in each thread."""
    import torch
    from imagestitch_amd import _lib
    lib = _lib.load()
    LOOPS = 48
    plans = []
    for t, (kind, size, rnames) in enumerate(((P.FISHEYE, P.SIZES[0], ("identity", "yaw0.52")), (P.STEREOGRAPHIC, P.SIZES[0], ("pitch-pi/2", "identity")),
                                              (P.FISHEYE, P.SIZES[1], ("pitch+pi/2", "pitch+pi/3")), (P.STEREOGRAPHIC, P.SIZES[1], ("yaw0.52", "pitch-pi/2")))):
        rng = np.random.default_rng(300 + t)
        cams = []
        for rname in rnames:
            w, h, f, K, R = P.rig(size, rname)
            m = P.from_rig(kind, f, K, R)
            roi, mm = m.detect_roi(w, h)
            roi = tuple(int(v) for v in roi)
            win = _window(roi)
            xm, ym = m.build_maps(win)
            src = PC.image(rng, h, w)
            cams.append(dict(w=w, h=h, K=K, R=R, roi=roi, mm=mm, win=win, xm=xm, ym=ym, src=src, whole=win == roi,
                             wi=oracle.remap(src, xm, ym, PC.LINEAR, PC.REFLECT), wm=oracle.remap(np.full((h, w), 255, np.uint8), xm, ym, PC.NEAREST, PC.CONST)))
        plans.append(dict(kind=kind, f=float(size[2]), cams=cams, got=[]))
    assert any(c["whole"] for p in plans for c in p["cams"])
    start = threading.Barrier(len(plans))

    def work(errors, p):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                warper = (gpu.FisheyeWarper if p["kind"] == P.FISHEYE else gpu.StereographicWarper)(0, stream).create(p["f"])
                warper.set_roi_cache(False)
                srcs = [_dev(c["src"]) for c in p["cams"]]
                like = torch.empty(1, device="cuda")
                start.wait(timeout=60)
                for i in range(LOOPS):
                    k = i % 2
                    c = p["cams"][k]
                    roi, mm = warper.warpRoi((c["w"], c["h"]), c["K"], c["R"], with_minmax=True)
                    gx, gy = warper.buildMapsRoi(c["K"], c["R"], c["win"], like=like)
                    wi = warper.warp_roi(srcs[k], c["K"], c["R"], PC.LINEAR, PC.REFLECT, c["win"], torch.empty(c["wi"].shape, dtype=torch.uint8, device="cuda"))
                    fused = warper.warp_with_mask(srcs[k], c["K"], c["R"]) if c["whole"] else None       # (finds the ROI itself: another scan)
                    assert lib.isx_last_error() in (b"",), lib.isx_last_error()
                    p["got"].append((k, roi, mm, gx, gy, wi, fused))
            stream.synchronize()
        except BaseException as ex:       # noqa: BLE001
            errors.append(ex)

    errors = []
    ts = [threading.Thread(target=work, args=(errors, p)) for p in plans]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "a thread did not finish"
    if errors:
        raise errors[0]
    torch.cuda.synchronize()
    for p in plans:
        assert len(p["got"]) == LOOPS
        for k, roi, mm, gx, gy, wi, fused in p["got"]:
            c = p["cams"][k]
            assert roi == c["roi"] and np.array_equal(mm, c["mm"]), (p["kind"], roi, c["roi"])
            assert PC.same_bits(_np(gx), c["xm"]) and PC.same_bits(_np(gy), c["ym"]) and np.array_equal(_np(wi), c["wi"])
            if fused is not None:
                assert fused[0] == c["roi"][:2] and np.array_equal(_np(fused[1]), c["wi"]) and np.array_equal(_np(fused[2]), c["wm"])


# ---- d. the ROI memo past its size --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_roi_memo_past_1024_entries(gpu, kind):
    """1100 distinct cameras (a yaw / pitch grid) on an 8 x 6 source with the ROI cache on: the memo the polar kinds share with the
    cylindrical kind holds 1024, so the first 76 are forgotten by the end.  Every answer - scanned, remembered, scanned again after
    eviction, with the cache switched off, and for a second source size on the same cameras - equals the model's."""
    f = 9.0
    sizes = ((8, 6), (7, 9))
    K = np.array([[f, 0, 4.0], [0, f, 3.0], [0, 0, 1]], F)
    cams = [(K, (P.rot("y", -1.2 + 0.06 * (i % 40)) @ P.rot("x", -0.7 + 0.05 * (i // 40))).astype(F)) for i in range(1100)]
    want = {(sz, i): P.from_rig(kind, f, Kc, Rc).detect_roi(*sz) for sz in sizes for i, (Kc, Rc) in enumerate(cams)}      # computed once
    assert len({tuple(R.ravel()) for _, R in cams}) == 1100
    warper = _warper(gpu, kind, f)
    warper.set_roi_cache(True)

    def ask(sz, i):
        roi, mm = warper.warpRoi(sz, cams[i][0], cams[i][1], with_minmax=True)
        mroi, mmm = want[(sz, i)]
        assert roi == tuple(int(v) for v in mroi) and np.array_equal(mm, mmm), (sz, i, roi, mroi, mm, mmm)

    for i in range(1100):
        ask(sizes[0], i)
    for i in list(range(80)) + list(range(1020, 1100)):       # the first 76 were evicted (scanned again), the rest are remembered
        ask(sizes[0], i)
    for i in range(1100):                                     # the same cameras at another size never hit the first size's entries
        ask(sizes[1], i)
    for i in (0, 1099):
        ask(sizes[0], i)
    warper.set_roi_cache(False)
    for i in (5, 5, 1099, 5):
        ask(sizes[0], i)
        ask(sizes[1], i)
