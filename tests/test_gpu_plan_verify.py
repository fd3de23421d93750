"""The device-side verification of planned warps (k_roi_border_sph / k_roi_scan -> k_roi_check_rearm -> isx_warper_plan_status) against the
three-valued model of tests/helpers/plan_verify_np.py over the cameras of tests/plan_verify_cases.py: it must FLAG every stale plan the model
says it must - each of the four bounds shifted up and down, over every scan kind, pole, sign of bound and the back seam - and pass every
right one, through every route a plan takes into the verifier.  The COUNT is read (isx_warper_plan_status's *mismatches, as deltas: the
counter is sticky), not only the error code.  tests/test_plan_verify_model.py holds the model and the case list to their own contract on
the CPU (every true plan MUST_PASS, at most 10 % of the shifted plans NO_CLAIM), so nothing here hides behind plans nobody asserts on."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_verify_cases as PC  # noqa: E402
from helpers import plan_verify_np as M  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_PLAN = 8
IDS = [PC.case_id(c) for c in PC.CASES]
SCAN_NAMES = {"roi_border", "roi_border_sph", "roi_scan"}


def status(w):
    """isx_warper_plan_status -> (return code, *mismatches)"""
    n = C.c_int(-1)
    rc = w._lib.isx_warper_plan_status(w._h, C.byref(n))
    assert rc in (0, ERR_PLAN), rc
    assert (rc == 0) == (n.value == 0), (rc, n.value)
    return rc, n.value


def count(w):
    return status(w)[1]


def make(gpu, case):
    kind, scale, K, R, sw, sh = PC.camera(case)
    w = (gpu.CylindricalWarper() if kind == M.CYL else gpu.SphericalWarper()).create(scale)
    return w, K, R, (sw, sh)


def index_of(cls, size=None, kind=None):
    for i, c in enumerate(PC.CASES):
        if c[0] == cls and (size is None or (c[2], c[3]) == size) and (kind is None or c[1] == kind):
            return i
    raise KeyError((cls, size, kind))


def true_and_stale(oracle, i, shift=(0, -1)):
    t = PC.truth(oracle, i)
    j = 1 + M.SHIFTS.index(shift)
    assert t["verdicts"][0][0] == M.MUST_PASS and t["verdicts"][j][0] == M.MUST_FLAG
    return t["plans"][0][1], t["plans"][j][1]


# ---- every bound, shifted up and down, one plan at a time --------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=IDS)
def test_shifts_one_at_a_time(gpu, oracle, i):
    """queue_verify -> verify -> plan_status for the true plan and each of its eight +-1 shifts: the count rises by 0 where the model says
    MUST_PASS and by exactly 1 where it says MUST_FLAG; what it makes no claim about is run and printed."""
    w, K, R, size = make(gpu, PC.CASES[i])
    t = PC.truth(oracle, i)
    before, wrong = count(w), []
    assert before == 0
    for (shift, plan), (verdict, per) in zip(t["plans"], t["verdicts"]):
        w.queue_verify(size, K, R, plan)
        w.verify()
        now = count(w)
        delta, before = now - before, now
        print(PC.case_id(PC.CASES[i]), "shift", shift, "plan", plan, verdict, per, "delta", delta)
        if (verdict == M.MUST_PASS and delta != 0) or (verdict == M.MUST_FLAG and delta != 1) or delta not in (0, 1):
            wrong.append((shift, plan, verdict, per, delta))
    assert not wrong, (t["roi"], t["extrema"], wrong)


# ---- the same nine behind one another in ONE flush: the keys are re-armed between consecutive checks --------------------------------------
@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=IDS)
def test_pending_batch_in_one_flush(gpu, oracle, i):
    w, K, R, size = make(gpu, PC.CASES[i])
    t = PC.truth(oracle, i)
    for _shift, plan in t["plans"]:
        w.queue_verify(size, K, R, plan)
    w.verify()
    verdicts = [v for v, _per in t["verdicts"]]
    got = count(w)
    assert verdicts.count(M.MUST_FLAG) <= got <= verdicts.count(M.MUST_FLAG) + verdicts.count(M.NO_CLAIM), (got, verdicts)


def test_rearm_between_wide_and_narrow(gpu, oracle):
    """A wide camera's extrema must not outlive its check: a narrow camera's true plan queued behind it in the same flush, whose extrema
    lie strictly inside the wide one's, passes only if the four shared keys were re-armed in between."""
    for kind, mk in ((M.CYL, gpu.CylindricalWarper), (M.SPH, gpu.SphericalWarper)):
        scale = 173.0
        K_w, R_w, size_w = np.array([[157.3, 0, 126.2], [0, 157.3, 62.6], [0, 0, 1]], np.float32), PC.rotation(0.3, -0.176, -0.006), (256, 128)
        K_n, R_n, size_n = np.array([[160.0, 0, 16.3], [0, 160.0, 16.6], [0, 0, 1]], np.float32), PC.rotation(0.25, -0.15, 0.01), (33, 33)
        tw = M.truth(oracle, kind, scale, K_w, R_w, *size_w)
        tn = M.truth(oracle, kind, scale, K_n, R_n, *size_n)
        for t in (tw, tn):
            assert M.verdict(kind, scale, t["roi"], t["extrema"])[0] == M.MUST_PASS
        ew, en = tw["extrema"], tn["extrema"]
        assert ew[0] + 2 < en[0] and ew[1] + 2 < en[1] and en[2] < ew[2] - 2 and en[3] < ew[3] - 2, (ew, en)
        w = mk().create(scale)
        for size, K, R, t in ((size_w, K_w, R_w, tw), (size_n, K_n, R_n, tn), (size_w, K_w, R_w, tw)):
            w.queue_verify(size, K, R, t["roi"])
        w.verify()
        assert status(w) == (0, 0), kind
        stale = M.shifted(tn["roi"], 3, 1)
        assert M.verdict(kind, scale, stale, tn["extrema"])[0] == M.MUST_FLAG
        for size, K, R, plan in ((size_w, K_w, R_w, tw["roi"]), (size_n, K_n, R_n, stale), (size_w, K_w, R_w, tw["roi"])):
            w.queue_verify(size, K, R, plan)
        w.verify()
        assert status(w) == (ERR_PLAN, 1), kind


# ---- every route into the verifier --------------------------------------------------------------------------------------------------------
ROUTE_CASES = [index_of("cyl_light", (256, 128)), index_of("cyl_rolled", (256, 128)), index_of("sph_plain", (256, 128))]


def _warp_planned(w, img, K, R, plan):
    import torch
    h, wd = plan[3] - plan[1] + 1, plan[2] - plan[0] + 1
    dst = torch.empty((h, wd, 3), dtype=torch.uint8, device=img.device)
    dmask = torch.empty((h, wd), dtype=torch.uint8, device=img.device)
    w.warp_with_mask_planned(img, K, R, plan, dst, dmask)
    return dst, dmask


@pytest.mark.parametrize("i", ROUTE_CASES, ids=[IDS[i] for i in ROUTE_CASES])
def test_routes_true_then_stale(gpu, oracle, i):
    """One true and one stale plan through each route: the immediate planned warp, set_deferred_verify + verify, verify_after(event), a
    begin_batch / end_batch pair, set_stream between queueing and verify, and discard_pending (what is dropped is never counted)."""
    import torch
    dev = torch.device("cuda:0")
    true, stale = true_and_stale(oracle, i)
    w, K, R, size = make(gpu, PC.CASES[i])
    img = torch.from_numpy(np.random.default_rng(i).integers(0, 256, (size[1], size[0], 3)).astype(np.uint8)).to(dev)
    keep, n = [], 0

    def expect(delta, route):
        nonlocal n
        got = count(w)
        assert got - n == delta, (route, got, n, delta)
        n = got

    # the immediate planned warp
    keep.append(_warp_planned(w, img, K, R, true)); expect(0, "immediate, true")
    keep.append(_warp_planned(w, img, K, R, stale)); expect(1, "immediate, stale")
    # deferred: nothing runs before verify(); plan_status itself starts what is still queued
    w.set_deferred_verify(True)
    keep.append(_warp_planned(w, img, K, R, true)); w.verify(); expect(0, "deferred, true")
    keep.append(_warp_planned(w, img, K, R, stale)); w.verify(); expect(1, "deferred, stale")
    keep.append(_warp_planned(w, img, K, R, stale)); expect(1, "deferred, stale, started by plan_status")
    # verify_after(event)
    for plan, delta in ((true, 0), (stale, 1)):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        w.queue_verify(size, K, R, plan)
        w.verify_after(ev)
        expect(delta, "verify_after")
        keep.append(ev)
    w.set_deferred_verify(False)
    # inside a batch: the verifications start when it ends
    w.begin_batch()
    keep.append(_warp_planned(w, img, K, R, true)); keep.append(_warp_planned(w, img, K, R, stale)); keep.append(_warp_planned(w, img, K, R, true))
    w.end_batch()
    expect(1, "batch of true, stale, true")
    # the handle changes its stream between queueing and verify
    s = torch.cuda.Stream(device=dev)
    for plan, delta in ((true, 0), (stale, 1)):
        w.queue_verify(size, K, R, plan)
        w.set_stream(s)
        w.verify()
        expect(delta, "set_stream before verify")
        w.set_stream(None)
    # a stale plan queued and dropped
    w.queue_verify(size, K, R, stale)
    w.discard_pending()
    w.verify()
    expect(0, "discard_pending")
    w.queue_verify(size, K, R, true)
    w.verify()
    assert status(w) == (ERR_PLAN, n) and n == 6
    torch.cuda.synchronize(dev)
    del w, keep


@pytest.mark.parametrize("i", ROUTE_CASES[:2], ids=[IDS[i] for i in ROUTE_CASES[:2]])
def test_captured_chain_counts_per_replay(gpu, oracle, i):
    """queue_verify + verify + join captured into a hipGraph (the verification forked inside the graph): a stale plan adds one per replay,
    a true one none."""
    import torch
    dev = torch.device("cuda:0")
    true, stale = true_and_stale(oracle, i)
    for plan, per_replay in ((true, 0), (stale, 1)):
        w, K, R, size = make(gpu, PC.CASES[i])
        gs = torch.cuda.Stream(device=dev)
        w.set_stream(gs)
        gs.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(gs):          # warm-up: the side stream, its events and the keys exist before the capture
            w.queue_verify(size, K, R, true)
            w.verify()
            w.join()
        torch.cuda.synchronize(dev)
        assert status(w) == (0, 0)
        gc.collect()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=gs, capture_error_mode="relaxed"):
            w.queue_verify(size, K, R, plan)
            w.verify()
            w.join()
        assert count(w) == 0, "capturing runs nothing"
        for r in range(1, 4):
            graph.replay()
            torch.cuda.synchronize(dev)
            assert count(w) == per_replay * r, (plan, r)
        w.set_stream(None)
        del graph, w


def test_two_handles_share_the_side_stream(gpu, oracle):
    """Every warper of a device runs its verifications on one shared stream, each with keys and a counter of its own: interleaved true and
    stale plans of two handles are counted per handle."""
    ia, ib = index_of("cyl_corner_behind", (256, 128)), index_of("sph_north", (257, 129))
    (wa, Ka, Ra, sa), (wb, Kb, Rb, sb) = make(gpu, PC.CASES[ia]), make(gpu, PC.CASES[ib])
    ta, sta = true_and_stale(oracle, ia)
    tb, stb = true_and_stale(oracle, ib, (3, -1))
    wa.queue_verify(sa, Ka, Ra, sta); wa.verify()
    wb.queue_verify(sb, Kb, Rb, tb); wb.verify()
    wa.queue_verify(sa, Ka, Ra, ta); wb.queue_verify(sb, Kb, Rb, stb)
    wa.verify(); wb.verify()
    wb.queue_verify(sb, Kb, Rb, stb); wa.queue_verify(sa, Ka, Ra, ta)
    wb.verify(); wa.verify()
    wb.queue_verify(sb, Kb, Rb, tb); wb.verify()
    assert status(wa) == (ERR_PLAN, 1)
    assert status(wb) == (ERR_PLAN, 2)
    wc, Kc, Rc, sc = make(gpu, PC.CASES[ia])          # a third handle on the same stream starts clean
    wc.queue_verify(sc, Kc, Rc, ta); wc.verify()
    assert status(wc) == (0, 0)


def test_flag_is_sticky_and_a_fresh_handle_is_clean(gpu, oracle):
    i = index_of("sph_plain", (33, 33))
    true, stale = true_and_stale(oracle, i, (1, 1))
    w, K, R, size = make(gpu, PC.CASES[i])
    assert status(w) == (0, 0)                        # nothing queued, nothing allocated
    w.queue_verify(size, K, R, true); w.verify()
    assert status(w) == (0, 0)
    w.queue_verify(size, K, R, stale); w.verify()
    assert status(w) == (ERR_PLAN, 1)
    for _ in range(3):
        w.queue_verify(size, K, R, true); w.verify()
        assert status(w) == (ERR_PLAN, 1)
    with pytest.raises(gpu.IsxError) as e:
        w.plan_status()
    assert e.value.code == ERR_PLAN
    del e
    w2, _, _, _ = make(gpu, PC.CASES[i])
    assert status(w2) == (0, 0)


# ---- which scan a camera gets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=IDS)
def test_verify_is_light_and_the_scan_launched(gpu, oracle, i):
    from imagestitch_amd import _lib
    w, K, R, size = make(gpu, PC.CASES[i])
    t = PC.truth(oracle, i)
    scan = t["scan"][0]
    assert w.verify_is_light(size, K, R) == (scan != "roi_scan"), t["scan"]
    lib = _lib.load()
    lib.isx_profile_enable(1); lib.isx_profile_filter(None); lib.isx_profile_sample(1); lib.isx_profile_reset()
    try:
        w.queue_verify(size, K, R, t["roi"])
        w.verify()
        assert status(w) == (0, 0)
        names = set(_lib.profile_entries())
    finally:
        lib.isx_profile_enable(0)
    assert names & SCAN_NAMES == {scan} and "roi_check" in names, (names, scan)
