"""Long-lived handles: the state one warper or blender carries from call to call, which the parity suite's one-call-per-fresh-handle cases
never cross.

- the warper's mapBackward table arena starting over (1024 entries, 16 MiB) and its ROI memos evicting, every warp against the oracle;
- a captured step whose warp tables the arena would reuse after a start-over, and a warp that misses its table while the stream is captured;
- the blender's device tile table across a stream change between a capture and its replays;
- a blender that outgrows its buffers after a capture (the old allocations are kept for the graph);
- a warp that fails inside a batch, a handle destroyed with a batch open;
- the narrowed-copies decision of a cycle whose first tile is not narrowed;
- four host threads in the library at once (ctypes releases the GIL), and isx_last_error per thread.

Every output is compared bit for bit with the oracle; where a replay is compared with the handle's own eager output, that eager output is
compared with the oracle in the same test."""
import gc
import threading

import numpy as np
import pytest

from imagestitch_amd import synth

pytestmark = pytest.mark.gpu

CYL, SPH = 0, 1
NEAREST, LINEAR = 0, 1
CONST, REFLECT = 0, 2
I16, F32, F16 = 0, 1, 2
ERR_STATE, ERR_SIZE, ERR_INVALID = 3, 7, 1


def _K(w, h, f):
    return np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]], np.float32)


def _R(yaw, pitch, roll=0.003):
    return (synth._rot("y", yaw) @ synth._rot("x", pitch) @ synth._rot("z", roll)).astype(np.float32)


def _warper(gpu, kind, f):
    return (gpu.CylindricalWarper if kind == CYL else gpu.SphericalWarper)().create(f)


def _check_warp(oracle, warper, kind, f, K, R, src_np, src_dev):
    """warp() on the device (ROI scan + table + remap) against the oracle's W:145-161; returns the warped tile's key (corner, size)."""
    corner, dst = warper.warp(src_dev, K, R, LINEAR, REFLECT)
    oc, od, _ = oracle.warp_u8(kind, f, K, R, src_np, LINEAR, REFLECT)
    got = dst.cpu().numpy()
    assert corner == oc and got.shape == od.shape, (corner, oc, got.shape, od.shape)
    assert np.array_equal(got, od), np.argwhere(got != od)[:4]
    return corner, od.shape[:2]


def _oracle_pair_step(oracle, p, bands, prec, out_f32):
    """What a PairStitcher step must give: the oracle's warps of every tile (checked against the stitcher's own warped tiles), the seam
    masks the stitcher uses, the oracle's MultiBandBlender."""
    ob = oracle.MultiBand(bands, prec)
    ob.prepare(p.corners, p.sizes)
    for i in p.active:
        src = p.imgs[i].cpu().numpy()
        oc, owi, _ = oracle.warp_u8(p.warper_kind, p.scale, p.K, p.Rs[i], src, LINEAR, REFLECT)
        _, owm, _ = oracle.warp_u8(p.warper_kind, p.scale, p.K, p.Rs[i], np.full(src.shape[:2], 255, np.uint8), NEAREST, CONST)
        assert oc == tuple(p.corners[i])
        assert np.array_equal(p.warped[i].cpu().numpy(), owi) and np.array_equal(p.wmasks[i].cpu().numpy(), owm)
        ob.feed(owi.astype(np.int16), p.seam[i].cpu().numpy(), p.corners[i])
    return ob.blend(out_f32)


def _stitcher(gpu, imgs, K, Rs, f, kind, bands, prec):
    from imagestitch_amd.pipeline import PairStitcher
    p = PairStitcher(imgs, K, Rs, f, "cylindrical" if kind == CYL else "spherical", bands, prec, 0, None, "int16")
    p.warper_kind, p.scale, p.imgs = kind, f, imgs
    return p


# ---- 1. the warper's table arena and ROI memos ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roi_cache", [False, True])
@pytest.mark.parametrize("kind", [CYL, SPH])
def test_table_arena_starts_over_past_1024_entries(gpu, oracle, kind, roi_cache):
    """More than 1024 distinct ROIs through one handle (small, short sources): the arena starts over on its entry count; the ROI memos
    (1 entry, or 1024 with set_roi_cache; spherical 64 / 1024) evict their oldest entries on the way.  Every warp equals the oracle's, and so
    do the first ROIs warped again after the start-over and the evictions."""
    import torch
    w, h, f = 64, 10, 300.0
    K = _K(w, h, f)
    rng = np.random.default_rng(40 + kind + 2 * int(roi_cache))
    src = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    src_dev = torch.from_numpy(src).cuda()
    warper = _warper(gpu, kind, f)
    warper.set_roi_cache(roi_cache)
    seen, cams = set(), []
    r0 = warper.table_resets()
    i = 0
    while len(seen) < 1100:
        R = _R(-0.9 + 0.0031 * (i % 600), -0.2 + 0.011 * (i // 600) + 0.0007 * (i % 7))
        seen.add(_check_warp(oracle, warper, kind, f, K, R, src, src_dev))
        cams.append(R)
        i += 1
    assert warper.table_resets() >= r0 + 1, "1100 distinct ROIs did not start the table arena over"
    for R in cams[:40] + cams[-5:]:
        _check_warp(oracle, warper, kind, f, K, R, src, src_dev)


@pytest.mark.parametrize("kind", [CYL, SPH])
def test_table_arena_starts_over_past_16_mib(gpu, oracle, kind):
    """Wide, short sources: ~75 KB of column tables per ROI fill the 16 MiB arena long before 1024 entries; every warp equals the oracle's
    before and after the start-over, and the first ROIs again after it."""
    import torch
    w, h, f = 12000, 6, 6000.0
    K = _K(w, h, f)
    rng = np.random.default_rng(7 + kind)
    src = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    src_dev = torch.from_numpy(src).cuda()
    warper = _warper(gpu, kind, f)
    r0 = warper.table_resets()
    cams, seen = [], set()
    i = 0
    while warper.table_resets() == r0:
        assert i < 600, "the byte limit was never reached"
        R = _R(-0.3 + 0.0011 * i, 0.02)
        seen.add(_check_warp(oracle, warper, kind, f, K, R, src, src_dev))
        cams.append(R)
        i += 1
    assert len(seen) < 1024, "the start-over came from the entry count, not the bytes"
    for R in cams[:8] + [_R(0.25 + 0.001 * j, -0.01) for j in range(8)]:
        _check_warp(oracle, warper, kind, f, K, R, src, src_dev)
    assert warper.table_resets() == r0 + 1


# ---- 2. warp tables under a captured graph ---------------------------------------------------------------------------------------------------
def test_captured_step_survives_a_table_start_over(gpu, oracle):
    """A PairStitcher step captured into a hipGraph holds raw pointers to its warps' tables.  Eager warps of 1100 other ROIs through the same
    warper (each equal to the oracle's) start its table arena over; the chunks the graph reads must not be rewritten: the replay still equals
    the pre-capture step, which equals the oracle."""
    import torch
    W, H, F = 320, 200, 260.0
    K, Rs = synth.camera_pair(W, H, F)
    imgs = [torch.from_numpy(synth.make_tile(H, W, i)).cuda() for i in range(2)]
    p = _stitcher(gpu, imgs, K, Rs, F, CYL, 4, F32)
    ref = [t.clone() for t in p.step()]
    torch.cuda.synchronize()
    od, om = _oracle_pair_step(oracle, p, 4, F32, False)
    assert np.array_equal(ref[0].cpu().numpy(), od) and np.array_equal(ref[1].cpu().numpy(), om)
    p.capture()
    out, m = p.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(m, ref[1])
    src = synth.make_tile(8, 48, 9, noise_only=True)
    with torch.cuda.stream(p.gstream):
        src_dev = torch.from_numpy(src).cuda()
        K2 = _K(48, 8, F)
        seen = set()
        i = 0
        while len(seen) < 1100:
            seen.add(_check_warp(oracle, p.warper, CYL, F, K2, _R(-0.8 + 0.005 * (i % 320), -0.3 + 0.02 * (i // 320)), src, src_dev))
            i += 1
    torch.cuda.synchronize()
    for _ in range(2):
        out, m = p.replay()
    torch.cuda.synchronize()
    assert torch.equal(m, ref[1])
    assert torch.equal(out, ref[0]), "the replay read tables the arena had given to other ROIs"
    assert p.warper.table_resets() >= 1
    assert p.check_plan() == 0


def test_table_miss_while_capturing_is_refused(gpu):
    """A fresh warper on a stream being captured: its table is not cached, and building it needs a host synchronisation the capture cannot
    hold - ISX_ERR_STATE before anything is enqueued, the capture itself stays valid."""
    import torch
    W, H, F = 160, 90, 140.0
    K, Rs = synth.camera_pair(W, H, F)
    img = torch.from_numpy(synth.make_tile(H, W, 1)).cuda()
    warper = gpu.CylindricalWarper().create(F)
    roi = warper.warpRoi((W, H), K, Rs[0])
    dh, dw = roi[3] - roi[1] + 1, roi[2] - roi[0] + 1
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    warper.set_stream(s)
    with torch.cuda.stream(s):
        dst = torch.zeros((dh, dw, 3), dtype=torch.uint8, device="cuda")
        dmask = torch.zeros((dh, dw), dtype=torch.uint8, device="cuda")
        x = torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    # a CUDAGraph that a dead reference cycle still holds (a test frame kept by its own pytest.raises info) must not be freed by a collection
    # that happens to run inside this capture: its destructor synchronises the device, which a capturing stream turns into an abort
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(gpu.IsxError) as e:
            warper.warp_with_mask_planned(img, K, Rs[0], roi, dst, dmask)
    assert e.value.code == ERR_STATE and "capture" in e.value.msg, e.value.msg
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    assert int(dst.abs().sum()) == 0 and int(dmask.sum()) == 0


# ---- 3. the blender's tile table across a stream change -------------------------------------------------------------------------------------
def _ring(gpu, n, seed, W=640, H=360, F=1800.0, bands=4, prec=F32):
    import torch
    K, Rs = synth.camera_ring(W, H, F, n, 0.17)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    imgs = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(n)]
    return _stitcher(gpu, imgs, K, Rs, F, CYL, bands, prec)


def _oracle_cycle(oracle, bands, prec, tiles, corners, sizes):
    ob = oracle.MultiBand(bands, prec)
    ob.prepare(corners, sizes)
    for (img, mask), c in zip(tiles, corners):
        ob.feed(img.astype(np.int16), mask, c)
    return ob.blend(True)


def test_blender_table_survives_a_stream_change_between_capture_and_replay(gpu, oracle):
    """test_gpu_many_tiles' capture / eager / replay / eager sequence with the blender moved to another stream after the capture: the stream
    change must not make the blender forget that the graph rewrites its tile table (the second eager blend trusted its mirror and read the
    captured step's tables)."""
    import torch
    p = _ring(gpu, 24, 5)
    ref = [t.clone() for t in p.step()]
    torch.cuda.synchronize()
    assert p.blender.last_path()["cycle"] == "deferred_table"
    od0, om0 = _oracle_pair_step(oracle, p, 4, F32, False)
    assert np.array_equal(ref[0].cpu().numpy(), od0) and np.array_equal(ref[1].cpu().numpy(), om0)
    p.capture()
    out, m = p.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(m, ref[1])
    corners = [(c[0] + 2 * i, c[1]) for i, c in enumerate(p.corners)]
    tiles = [(p.warped[i].cpu().numpy(), p.seam[i].cpu().numpy()) for i in range(24)]
    od, om = _oracle_cycle(oracle, 4, F32, tiles, corners, p.sizes)
    other = torch.cuda.Stream()
    other.wait_stream(p.gstream)
    p.blender.set_stream(other)

    def eager():
        with torch.cuda.stream(other):
            p.blender.prepare(corners, p.sizes)
            for i in range(24):
                p.blender.feed_u8(p.warped[i], p.seam[i], corners[i])
            d, mm = p.blender.blend(out_f32=True)
        torch.cuda.synchronize()
        assert p.blender.last_path()["cycle"] == "deferred_table"
        return d.cpu().numpy(), mm.cpu().numpy()

    for rep in range(2):
        d, mm = eager()
        assert np.array_equal(mm, om), rep
        assert np.array_equal(d, od), ("eager blend %d after the stream change differs from the oracle" % rep, np.argwhere(d != od)[:4])
        out, m = p.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref[0]) and torch.equal(m, ref[1]), rep


# ---- 4. growth after capture ------------------------------------------------------------------------------------------------------------------
def test_blender_growth_after_capture_keeps_what_the_graph_uses(gpu, oracle):
    """A captured 24-tile step, then an eager cycle of the same blender with more tiles, a larger panorama and more bands: its buffers grow.
    The allocations they outgrow are kept for the graph (retained_bytes > 0 before the replay), the eager cycle equals the oracle and the
    replay the pre-capture step."""
    import torch
    p = _ring(gpu, 24, 11)
    ref = [t.clone() for t in p.step()]
    torch.cuda.synchronize()
    od0, om0 = _oracle_pair_step(oracle, p, 4, F32, False)
    assert np.array_equal(ref[0].cpu().numpy(), od0) and np.array_equal(ref[1].cpu().numpy(), om0)
    assert p.blender.retained_bytes() == 0
    p.capture()
    out, m = p.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(m, ref[1])
    rng = np.random.default_rng(12)
    n, bands = 40, 6
    corners, sizes, tiles = [], [], []
    x = 0
    for i in range(n):
        w, h = int(rng.integers(500, 700)), int(rng.integers(380, 460))
        corners.append((x, int(rng.integers(-20, 21))))
        sizes.append((w, h))
        x += int(w * rng.uniform(0.4, 0.7))
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        mask = (rng.random((h, w)) > 0.1).astype(np.uint8) * 255
        tiles.append((img, mask))
    od, om = _oracle_cycle(oracle, bands, F32, tiles, corners, sizes)
    with torch.cuda.stream(p.gstream):
        dev = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in tiles]
        p.blender.setNumBands(bands)
        p.blender.prepare(corners, sizes)
        for (ti, tm), c in zip(dev, corners):
            p.blender.feed_u8(ti, tm, c)
        d, mm = p.blender.blend(out_f32=True)
    torch.cuda.synchronize()
    assert np.array_equal(mm.cpu().numpy(), om) and np.array_equal(d.cpu().numpy(), od)
    assert p.blender.retained_bytes() > 0, "the grown buffers freed what the captured graph still uses"
    for _ in range(2):
        out, m = p.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(m, ref[1])


def test_blender_table_growth_after_capture_keeps_the_captured_table(gpu, oracle):
    """The growth case of the device tile table itself: a captured 24-tile step, then an eager cycle of 1200 small tiles inside the same
    panorama with the same bands.  Nothing of that cycle outgrows the captured step's pyramids or tile buffers (a smaller panorama, smaller
    tiles; tile slots past 24 are new allocations, not growths); only the tile table does - (2 L + 2) slots of ~1200 descriptors pass its
    1 MiB.  So the retained bytes are exactly the old table, the eager cycle equals the oracle and the replay the pre-capture step."""
    import torch
    p = _ring(gpu, 24, 17)
    ref = [t.clone() for t in p.step()]
    torch.cuda.synchronize()
    od0, om0 = _oracle_pair_step(oracle, p, 4, F32, False)
    assert np.array_equal(ref[0].cpu().numpy(), od0) and np.array_equal(ref[1].cpu().numpy(), om0)
    p.capture()
    out, m = p.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(m, ref[1])
    assert p.blender.retained_bytes() == 0
    fw = p.mosaic_size[0]
    x0, y0 = min(c[0] for c in p.corners), min(c[1] for c in p.corners)
    rng = np.random.default_rng(18)
    n = 1200
    sizes = [(int(rng.integers(10, 20)), int(rng.integers(6, 12))) for _ in range(n)]
    corners = [(x0 + int(rng.integers(0, fw - 40)), y0 + int(rng.integers(0, 200))) for _ in range(n)]
    tiles = [(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), (rng.random((h, w)) > 0.2).astype(np.uint8) * 255) for (w, h) in sizes]
    od, om = _oracle_cycle(oracle, 4, F32, tiles, corners, sizes)
    with torch.cuda.stream(p.gstream):
        dev = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in tiles]
        p.blender.prepare(corners, sizes)
        for (ti, tm), c in zip(dev, corners):
            p.blender.feed_u8(ti, tm, c)
        d, mm = p.blender.blend(out_f32=True)
    torch.cuda.synchronize()
    assert p.blender.last_path()["cycle"] == "deferred_table"
    assert np.array_equal(mm.cpu().numpy(), om) and np.array_equal(d.cpu().numpy(), od)
    assert p.blender.retained_bytes() == 1 << 20, "not exactly the old 1 MiB tile table was kept: %d" % p.blender.retained_bytes()
    for _ in range(2):
        out, m = p.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(m, ref[1])


# ---- 5. batch state -------------------------------------------------------------------------------------------------------------------------
def _batch_case(gpu, oracle):
    import torch
    W, H, F = 200, 120, 170.0
    K, Rs = synth.camera_ring(W, H, F, 3, 0.3)
    srcs = [synth.make_tile(H, W, 20 + i) for i in range(3)]
    devs = [torch.from_numpy(s).cuda() for s in srcs]
    warper = gpu.CylindricalWarper().create(F)
    outs = []
    for i in range(3):
        roi = warper.warpRoi((W, H), K, Rs[i])
        dh, dw = roi[3] - roi[1] + 1, roi[2] - roi[0] + 1
        dst = torch.full((dh, dw, 3), 77, dtype=torch.uint8, device="cuda")
        dmask = torch.full((dh, dw), 77, dtype=torch.uint8, device="cuda")
        oc, owi, _ = oracle.warp_u8(CYL, F, K, Rs[i], srcs[i], LINEAR, REFLECT)
        _, owm, _ = oracle.warp_u8(CYL, F, K, Rs[i], np.full((H, W), 255, np.uint8), NEAREST, CONST)
        outs.append((dst, dmask, owi, owm))
    torch.cuda.synchronize()
    return warper, K, Rs, devs, outs


def _is_oracle(o):
    return np.array_equal(o[0].cpu().numpy(), o[2]) and np.array_equal(o[1].cpu().numpy(), o[3])


def test_a_failing_warp_ends_the_batch(gpu, oracle):
    """begin_batch, warp A, warp B into a wrong-size dst (ISX_ERR_SIZE): A - which returned OK - is written without end_batch, and the handle
    no longer collects (end_batch launches nothing: A's dst, refilled with a sentinel, keeps it through a later begin / warp C / end)."""
    import torch
    warper, K, Rs, devs, outs = _batch_case(gpu, oracle)
    warper.begin_batch()
    warper.warp_with_mask(devs[0], K, Rs[0], dst_img=outs[0][0], dst_mask=outs[0][1])
    bad = torch.empty((5, 5, 3), dtype=torch.uint8, device="cuda")
    bad_m = torch.empty((5, 5), dtype=torch.uint8, device="cuda")
    with pytest.raises(gpu.IsxError) as e:
        warper.warp_with_mask(devs[1], K, Rs[1], dst_img=bad, dst_mask=bad_m)
    assert e.value.code == ERR_SIZE
    torch.cuda.synchronize()
    assert _is_oracle(outs[0]), "a warp that returned ISX_OK before the failing one was never launched"
    warper.end_batch()
    outs[0][0].fill_(77)
    outs[0][1].fill_(77)
    torch.cuda.synchronize()
    warper.begin_batch()
    warper.warp_with_mask(devs[2], K, Rs[2], dst_img=outs[2][0], dst_mask=outs[2][1])
    warper.end_batch()
    torch.cuda.synchronize()
    assert _is_oracle(outs[2])
    assert bool((outs[0][0] == 77).all()) and bool((outs[0][1] == 77).all()), "a stale batch entry was launched again"


def test_destroy_launches_an_open_batch(gpu, oracle):
    """begin_batch, warp A, destroy: A returned OK, so its output is written."""
    import torch
    warper, K, Rs, devs, outs = _batch_case(gpu, oracle)
    warper.begin_batch()
    warper.warp_with_mask(devs[0], K, Rs[0], dst_img=outs[0][0], dst_mask=outs[0][1])
    warper._lib.isx_warper_destroy(warper._h)
    warper._h = None
    torch.cuda.synchronize()
    assert _is_oracle(outs[0]), "destroy dropped a collected warp"


# ---- 6. narrowed copies mid-cycle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["host_s16", "device_u8"])
def test_narrowing_is_decided_by_the_first_tile(gpu, oracle, first):
    """Can a cycle whose first tile is not narrowed narrow a later one?  No: feed() takes the first recorded tile's decision for every later
    tile (a CV_16SC3 device tile behind a host CV_16SC3 tile is not narrowed; behind a CV_8UC3 tile the cycle turns eager), so
    set_narrow_copies(False) in the middle of such a cycle is allowed, and the mosaic equals the oracle's.  A cycle whose first tile IS
    narrowed refuses it (ISX_ERR_STATE)."""
    import torch
    rng = np.random.default_rng(61)
    n = 5
    corners, sizes, tiles = [], [], []
    x = 0
    for i in range(n):
        w, h = int(rng.integers(90, 130)), int(rng.integers(70, 90))
        corners.append((x, int(rng.integers(-6, 7))))
        sizes.append((w, h))
        x += int(w * 0.6)
        tiles.append((rng.integers(0, 256, (h, w, 3)).astype(np.uint8), (rng.random((h, w)) > 0.1).astype(np.uint8) * 255))
    od, om = _oracle_cycle(oracle, 3, F32, tiles, corners, sizes)
    mb = gpu.MultiBandBlender(False, 3, F32)
    mb.set_deferred_level0("copy")
    mb.prepare(corners, sizes)
    for i, ((img, mask), c) in enumerate(zip(tiles, corners)):
        if i == 0 and first == "host_s16":
            mb.feed(img.astype(np.int16), mask, c)
        elif i == 0:
            mb.feed_u8(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda(), c)
        else:
            mb.feed(torch.from_numpy(img.astype(np.int16)).cuda(), torch.from_numpy(mask).cuda(), c)
        if i == 2:
            mb.set_narrow_copies(False)
    d, m = mb.blend(out_f32=True)
    assert mb.feed_path()["narrowed"] == "none"
    assert np.array_equal(m.cpu().numpy(), om) and np.array_equal(d.cpu().numpy(), od)
    # the other side of the invariant: a narrowed first tile, and the switch is refused until the cycle ends
    mb.set_narrow_copies(True)
    mb.prepare(corners, sizes)
    for i, ((img, mask), c) in enumerate(zip(tiles, corners)):
        mb.feed(torch.from_numpy(img.astype(np.int16)).cuda(), torch.from_numpy(mask).cuda(), c)
        if i == 2:
            with pytest.raises(gpu.IsxError) as e:
                mb.set_narrow_copies(False)
            assert e.value.code == ERR_STATE
    d, m = mb.blend(out_f32=True)
    assert mb.feed_path()["narrowed"] == "confirmed"
    assert np.array_equal(m.cpu().numpy(), om) and np.array_equal(d.cpu().numpy(), od)


# ---- 7. threads -----------------------------------------------------------------------------------------------------------------------------------
def _pair_expect(oracle, kind, W, H, F, seed, bands, prec):
    K, Rs = synth.camera_pair(W, H, F, yaw=0.3)
    srcs = [synth.make_tile(H, W, seed + i) for i in range(2)]
    corners, owis, owms = [], [], []
    for i in range(2):
        oc, owi, _ = oracle.warp_u8(kind, F, K, Rs[i], srcs[i], LINEAR, REFLECT)
        _, owm, _ = oracle.warp_u8(kind, F, K, Rs[i], np.full((H, W), 255, np.uint8), NEAREST, CONST)
        corners.append(oc); owis.append(owi); owms.append(owm)
    seam = synth.seam_masks(corners, owms)
    sizes = [(m.shape[1], m.shape[0]) for m in owms]
    ob = oracle.MultiBand(bands, prec)
    ob.prepare(corners, sizes)
    for i in range(2):
        ob.feed(owis[i].astype(np.int16), seam[i], corners[i])
    od, om = ob.blend(prec != I16)
    return dict(kind=kind, F=F, K=K, Rs=Rs, srcs=srcs, corners=corners, owis=owis, owms=owms, seam=seam, sizes=sizes, bands=bands, prec=prec,
                od=od, om=om)


def _pair_steps(gpu, e, steps, errors):
    import torch
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            warper = (gpu.CylindricalWarper if e["kind"] == CYL else gpu.SphericalWarper)(0, stream).create(e["F"])
            mb = gpu.MultiBandBlender(False, e["bands"], e["prec"], 0, stream)
            srcs = [torch.from_numpy(s).cuda() for s in e["srcs"]]
            seam = [torch.from_numpy(s).cuda() for s in e["seam"]]
            for _ in range(steps):
                warped = []
                for i in range(2):
                    c, wi, wm = warper.warp_with_mask(srcs[i], e["K"], e["Rs"][i])
                    assert c == e["corners"][i]
                    warped.append((wi, wm))
                mb.prepare(e["corners"], e["sizes"])
                for i in range(2):
                    mb.feed_u8(warped[i][0], seam[i], e["corners"][i])
                d, m = mb.blend(out_f32=(e["prec"] != I16))
                stream.synchronize()
                for i in range(2):
                    assert np.array_equal(warped[i][0].cpu().numpy(), e["owis"][i]) and np.array_equal(warped[i][1].cpu().numpy(), e["owms"][i])
                assert np.array_equal(m.cpu().numpy(), e["om"]) and np.array_equal(d.cpu().numpy(), e["od"])
    except BaseException as ex:       # noqa: BLE001 - reported on the main thread
        errors.append(ex)


def _in_threads(fns):
    errors = []
    ts = [threading.Thread(target=f, args=(errors,)) for f in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "a thread did not finish"
    if errors:
        raise errors[0]


def test_four_threads_of_pair_steps_beside_seam_linear_and_gain(gpu, oracle):
    """Four threads, each with its own warper, blender and torch stream, different geometry, projection and precision, run 10 eager pair
    steps each, while three more threads run the DP seam finder, the linear pair blend and the gain estimate (thread-local scratch) and two
    warpers of one more thread share the per-device side and ROI streams with everyone.  Everything expected is computed here first."""
    import torch
    from oracle.dpseam_np import DpSeamFinder as OracleFinder
    from seam_cases import make_find_case
    from test_gain_model import feed_model
    exp = [_pair_expect(oracle, CYL, 320, 200, 260.0, 0, 5, I16), _pair_expect(oracle, SPH, 300, 180, 240.0, 4, 4, F32),
           _pair_expect(oracle, CYL, 256, 160, 300.0, 8, 3, F16), _pair_expect(oracle, SPH, 352, 208, 280.0, 12, 5, F32)]
    s_imgs, s_corners, s_masks = make_find_case(2001, 2, False, holes=True)
    s_ref = [m.copy() for m in s_masks]
    OracleFinder().find([im.astype(np.float32) for im in s_imgs], s_corners, s_ref)
    g = exp[0]
    g_model = feed_model(g["corners"], g["owis"], g["owms"])
    lrng = np.random.default_rng(17)
    l1 = lrng.random((120, 160, 3)).astype(np.float32) * 255
    l2 = lrng.random((123, 150, 3)).astype(np.float32) * 255
    l1[:15, -25:] = 3.0
    l2[-20:, :18] = 2.0
    ltl1, ltl2 = (10, 20), (105, 23)
    lrc, lpano, lseam = oracle.blend_pair_linear(l1, l2, ltl1, ltl2)
    assert lrc == 0

    def seams(errors):
        try:
            for _ in range(4):
                got = [m.copy() for m in s_masks]
                gpu.DpSeamFinder().find(s_imgs, s_corners, got)
                for a, b in zip(got, s_ref):
                    assert np.array_equal(a, b)
        except BaseException as ex:       # noqa: BLE001
            errors.append(ex)

    def gains(errors):
        try:
            for _ in range(6):
                comp = gpu.GainCompensator().feed(g["corners"], g["owis"], g["owms"])
                assert np.array_equal(comp.N, g_model[0]) and np.array_equal(comp.I.view(np.uint64), g_model[1].view(np.uint64))
        except BaseException as ex:       # noqa: BLE001
            errors.append(ex)

    def linear(errors):
        try:
            for _ in range(6):
                pano, seam = _gpu_pair_linear(l1, l2, ltl1, ltl2, lpano.shape)
                assert np.array_equal(seam, lseam) and np.array_equal(pano, lpano, equal_nan=True)
        except BaseException as ex:       # noqa: BLE001
            errors.append(ex)

    start = threading.Barrier(2)

    def planned_warper(errors, e):
        # one of two planned-warp handles, each in its own thread and on its own stream: both enqueue their verification scans on the
        # per-device side stream and take the per-device ROI stream at the same time (the static mutexes of warp.hip are contended)
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                w = gpu.CylindricalWarper(0, stream).create(e["F"])
                srcs = [torch.from_numpy(s).cuda() for s in e["srcs"]]
                start.wait(timeout=60)
                for _ in range(16):
                    for i in range(2):
                        roi = w.warpRoi((srcs[i].shape[1], srcs[i].shape[0]), e["K"], e["Rs"][i])
                        dh, dw = roi[3] - roi[1] + 1, roi[2] - roi[0] + 1
                        wi = torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda")
                        wm = torch.empty((dh, dw), dtype=torch.uint8, device="cuda")
                        w.warp_with_mask_planned(srcs[i], e["K"], e["Rs"][i], roi, wi, wm)
                        w.verify()
                        stream.synchronize()
                        assert np.array_equal(wi.cpu().numpy(), e["owis"][i]) and np.array_equal(wm.cpu().numpy(), e["owms"][i])
                assert w.plan_status() == 0
        except BaseException as ex:       # noqa: BLE001
            errors.append(ex)

    fns = [(lambda errors, e=e: _pair_steps(gpu, e, 10, errors)) for e in exp] + [seams, gains, linear]
    fns += [(lambda errors, e=e: planned_warper(errors, e)) for e in (exp[0], exp[2])]
    _in_threads(fns)


def _gpu_pair_linear(img1, img2, tl1, tl2, shape):
    """isx_blend_pair_linear on host mats (its scratch is thread_local)."""
    import ctypes as C
    from imagestitch_amd import _lib
    pano = np.empty(shape, np.float32)
    seam = np.zeros(shape[0], np.int32)
    m1, m2, mp = _lib.as_mat(img1), _lib.as_mat(img2), _lib.as_mat(pano)
    _lib.check(_lib.load().isx_blend_pair_linear(C.byref(m1), C.byref(m2), tl1[0], tl1[1], tl2[0], tl2[1], C.byref(mp),
                                                 seam.ctypes.data_as(_lib._IP), 0, None))
    return pano, seam


def test_last_error_is_per_thread(gpu):
    """A thread whose call fails on a host-side argument check reads its own message from isx_last_error, while the other threads' calls
    keep succeeding (and never see it)."""
    import torch
    msgs = []

    def failing(errors):
        try:
            for k in range(200):
                mb = gpu.MultiBandBlender(False, 3, F32)
                with pytest.raises(gpu.IsxError) as e:
                    mb.prepare([(0, 0), (5, 5)], [(10, 10), (0, 7)])
                assert e.value.code == ERR_INVALID and "tile 1 has empty size" in e.value.msg, e.value.msg
                msgs.append(e.value.msg)
        except BaseException as ex:       # noqa: BLE001
            errors.append(ex)

    def fine(errors):
        try:
            from imagestitch_amd import _lib
            lib = _lib.load()
            src = torch.from_numpy(synth.make_tile(60, 80, 3)).cuda()
            K, Rs = synth.camera_pair(80, 60, 70.0)
            for k in range(200):
                w = gpu.CylindricalWarper().create(70.0)
                w.warp_with_mask(src, K, Rs[k % 2])
                assert lib.isx_last_error() in (b"",), lib.isx_last_error()
        except BaseException as ex:       # noqa: BLE001
            errors.append(ex)

    _in_threads([failing, fine, fine])
    assert len(msgs) == 200
