"""The launch plan of the multi-band blender's host code, pinned against a recorded fixture (tests/golden/blend_plan.json).

For a fixed set of cycles - the pair whose last step is k_collapse_roll (planar / Q8 level 1) fed in four ways, a row whose tiles overlap their
second neighbours (more tiles over one strip than the rolling kernel has slots: k_collapse_gather and 16-byte records), three small ragged
tiles, a column window, batched chains, more than 20 tiles on the table and in column strips, side-stream chains, a mark
event, the eager cycle - the fixture holds what the host code decided: last_path(), level1_format(), feed_path(), the growth of table_uploads()
over a second identical cycle (more than 20 tiles), and per launch name the number of launches and the summed algorithmic bytes
(isx_profile_*).  Launches must match exactly; bytes to a relative 1e-9 - re-associating a few hundred double additions moves them by about
1e-13, the smallest real accounting change (one pixel's 3 bytes in the smallest tile here) by about 1e-4.  Every result is also compared with
the oracle, bit for bit.  Host-side refactors of blend.hip must leave all of it as it is.

    python tests/test_gpu_blend_plan.py --record      # rewrites the fixture from the library as built (on a GPU)
"""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "blend_plan.json")
I16, F32, F16 = 0, 1, 2
PREC = {I16: "i16", F32: "f32", F16: "f16"}
BYTES_RTOL = 1e-9

PAIR = ([(-40, 7), (233, -12)], [(411, 300), (397, 290)])
THREE_DEEP = ([(0, 0), (150, 9), (290, -6), (430, 4)], [(420, 260), (420, 255), (420, 262), (300, 250)])
RAGGED = ([(3, 1), (57, -2), (9, 77)], [(71, 93), (5, 140), (131, 33)])
WINDOW = ([(0, 0), (700, 11)], [(900, 400), (880, 390)])


def _tiles(rng, sizes):
    out = []
    for (w, h) in sizes:
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        mask = (rng.random((h, w)) > 0.2).astype(np.uint8) * 255
        mask[rng.random((h, w)) < 0.1] = 77
        out.append((img, mask))
    return out


def _row21(rng):
    corners, sizes, x = [], [], 0
    for _ in range(21):
        w, h = int(rng.integers(70, 120)), int(rng.integers(60, 90))
        corners.append((x, int(rng.integers(-8, 9))))
        sizes.append((w, h))
        x += int(w * rng.uniform(0.35, 0.8))
    return corners, sizes


def _stack21(rng):
    corners = [(int(rng.integers(0, 30)), 25 * i) for i in range(21)]
    sizes = [(int(rng.integers(80, 110)), 60) for _ in range(21)]
    return corners, sizes


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


def _oracle_blend(oracle, rig, tiles, bands, prec):
    corners, sizes = rig
    ob = oracle.MultiBand(bands, prec)
    ob.prepare(corners, sizes)
    for (img, mask), c in zip(tiles, corners):
        ob.feed(img.astype(np.int16), mask, c)      # the caller's convertTo(CV_16S)
    return ob.blend(prec != I16)


def _cycle(mb, rig, tiles, prec, feed="u8"):
    """prepare, feed every tile, blend.  feed: u8 = CV_8UC3 through feed_u8; s16 = CV_16SC3 through feed."""
    import torch
    corners, sizes = rig
    mb.prepare(corners, sizes)
    keep = []
    for (img, mask), c in zip(tiles, corners):
        ti = torch.from_numpy(img if feed == "u8" else img.astype(np.int16)).cuda()
        tm = torch.from_numpy(mask).cuda()
        keep.append((ti, tm))
        if feed == "u8":
            mb.feed_u8(ti, tm, c)
        else:
            mb.feed(ti, tm, c)
    d, m = mb.blend(out_f32=(prec != I16))
    return d.cpu().numpy(), m.cpu().numpy()


def _record_of(mb, prof, **more):
    rec = {"last_path": mb.last_path(), "level1_format": mb.level1_format(), "feed_path": mb.feed_path(), "launches": prof.launches}
    rec.update(more)
    return rec


def _single(gpu, oracle, rig, bands, prec, mode=True, feed="u8", seed=1, poke=False, window=None, overlap=False, mark=None, many=False, tab=None):
    """One cycle of one blender.  mode: set_deferred_level0's (None: the eager cycle); poke: one value 300 in the second tile (CV_16SC3 tiles that
    are not bytes); many: a second identical cycle, for the table's uploads; tab: ISX_TAB for the cycle (read per blend())."""
    import torch
    tiles = _tiles(np.random.default_rng(seed), rig[1])
    if poke:
        tiles = [(im.astype(np.int16), mk) for im, mk in tiles]
        tiles[1][0][7, 3, 1] = 300
    od, om = _oracle_blend(oracle, rig, tiles, bands, prec)
    old = os.environ.get("ISX_TAB")
    if tab is not None:
        os.environ["ISX_TAB"] = tab
    try:
        mb = gpu.MultiBandBlender(False, bands, prec)
        if mode is not None:
            mb.set_deferred_level0(mode)
        if overlap:
            mb.set_overlap(True)
        ev = None
        if mark is not None:
            ev = torch.cuda.Event()
            ev.record()      # materialise the hipEvent_t
            mb.set_mark_event(ev, mark)
        if window:
            mb.set_window(*window)
        with _Profile() as prof:
            d, m = _cycle(mb, rig, tiles, prec, feed)
        more = {}
        if many:
            u1 = mb.table_uploads()
            d2, m2 = _cycle(mb, rig, tiles, prec, feed)
            more["table_uploads_growth"] = mb.table_uploads() - u1
            assert np.array_equal(d2, d) and np.array_equal(m2, m)
        if ev is not None:
            torch.cuda.synchronize()
            assert ev.query()
    finally:
        if tab is not None:
            if old is None:
                os.environ.pop("ISX_TAB", None)
            else:
                os.environ["ISX_TAB"] = old
    if window:
        od, om = od[:, window[0]:window[1]], om[:, window[0]:window[1]]
    assert np.array_equal(m, om), np.argwhere(m != om)[:4]
    assert np.array_equal(d, od), np.argwhere(d != od)[:4]
    return _record_of(mb, prof, **more)


def _batch(gpu, oracle, nb, bands, prec):
    """blend_batch of nb pairs 330x210 + 300x220; the fixture's launches are the whole batch's, the paths those of every blender."""
    import torch
    from imagestitch_amd.blender import blend_batch
    rng = np.random.default_rng(40 + nb)
    bl, ds, ms, keep, want = [], [], [], [], []
    with _Profile() as prof:
        for q in range(nb):
            rig = ([(0, 0), (200 + q, 5)], [(330, 210), (300, 220)])
            tiles = _tiles(rng, rig[1])
            want.append(_oracle_blend(oracle, rig, tiles, bands, prec))
            mb = gpu.MultiBandBlender(False, bands, prec)
            mb.set_deferred_level0(True)
            mb.prepare(*rig)
            for (img, mask), c in zip(tiles, rig[0]):
                ti, tm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
                keep.append((ti, tm))
                mb.feed_u8(ti, tm, c)
            w, h = mb.result_size()
            bl.append(mb)
            ds.append(torch.empty((h, w, 3), dtype=torch.float32 if prec != I16 else torch.int16, device="cuda"))
            ms.append(torch.empty((h, w), dtype=torch.uint8, device="cuda"))
        blend_batch(bl, ds, ms)
    for q in range(nb):
        assert np.array_equal(ms[q].cpu().numpy(), want[q][1]) and np.array_equal(ds[q].cpu().numpy(), want[q][0]), q
    recs = [_record_of(mb, prof) for mb in bl]
    assert all(r == recs[0] for r in recs)
    return recs[0]


def _cases():
    c = {}
    # the pair: rolling last step, planar / Q8 level 1; fed by reference, with private copies (fused feed), as CV_16SC3 private copies that are
    # bytes (narrowed, confirmed) and that are not (widened)
    for bands in (2, 5, 7):
        for prec in (I16, F32, F16):
            for how, kw in (("ref_u8", dict(mode=True)), ("copy_u8", dict(mode="copy")), ("copy_s16", dict(mode="copy", feed="s16")),
                            ("copy_s16_300", dict(mode="copy", feed="s16", poke=True))):
                c["pair-%s-b%d-%s" % (PREC[prec], bands, how)] = lambda g, o, bands=bands, prec=prec, kw=kw: _single(g, o, PAIR, bands, prec, seed=11, **kw)
    c["three_deep-f32-b5"] = lambda g, o: _single(g, o, THREE_DEEP, 5, F32, seed=12)
    for prec in (I16, F32):
        for bands in (2, 5):
            c["ragged-%s-b%d" % (PREC[prec], bands)] = lambda g, o, bands=bands, prec=prec: _single(g, o, RAGGED, bands, prec, seed=13)
    c["window-f32-b5"] = lambda g, o: _single(g, o, WINDOW, 5, F32, seed=14, window=(256, 1024))
    for prec in (I16, F32):
        c["batch3-%s-b5" % PREC[prec]] = lambda g, o, prec=prec: _batch(g, o, 3, 5, prec)
        c["batch2-%s-b1" % PREC[prec]] = lambda g, o, prec=prec: _batch(g, o, 2, 1, prec)      # the last step is also the top
    row, stack = _row21(np.random.default_rng(15)), _stack21(np.random.default_rng(16))
    for prec in (I16, F32):
        for name, tab in (("table", None), ("strips", "0")):
            c["row21-%s-b4-%s" % (PREC[prec], name)] = lambda g, o, prec=prec, tab=tab: _single(g, o, row, 4, prec, seed=17, many=True, tab=tab)
            c["stack21-%s-b4-%s" % (PREC[prec], name)] = lambda g, o, prec=prec, tab=tab: _single(g, o, stack, 4, prec, seed=18, many=True, tab=tab)
    c["overlap-f32-b5"] = lambda g, o: _single(g, o, PAIR, 5, F32, seed=19, overlap=True)
    c["mark0-f32-b5-copy_u8"] = lambda g, o: _single(g, o, PAIR, 5, F32, seed=20, mode="copy", mark=0)      # the level-0 launch is skipped
    c["mark1-f32-b5-ref_u8"] = lambda g, o: _single(g, o, PAIR, 5, F32, seed=20, mark=1)
    for prec in (I16, F32):
        for bands in (0, 2):
            c["eager-%s-b%d" % (PREC[prec], bands)] = lambda g, o, bands=bands, prec=prec: _single(g, o, PAIR, bands, prec, seed=21, mode=None)
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_plan_equals_the_recorded_one(gpu, oracle, golden, case):
    got, want = CASES[case](gpu, oracle), golden[case]
    print(case, json.dumps(got, sort_keys=True))
    for key in ("last_path", "level1_format", "feed_path"):
        assert got[key] == want[key], (case, key, got[key], want[key])
    assert got.get("table_uploads_growth") == want.get("table_uploads_growth"), (case, got.get("table_uploads_growth"), want.get("table_uploads_growth"))
    assert sorted(got["launches"]) == sorted(want["launches"]), (case, sorted(got["launches"]), sorted(want["launches"]))
    for name, (n, by) in got["launches"].items():
        wn, wby = want["launches"][name]
        assert n == wn, (case, name, n, wn)
        assert abs(by - wby) <= BYTES_RTOL * abs(wby), (case, name, by, wby)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_blend_plan.py --record")
    sys.path.insert(0, ROOT)
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
