"""The features finder's per-thread scratch (ObScratch of csrc/orb.hip) across calls: a run of large, tiny, truncated and clean images on
one thread, on one stream and alternating two; a graph of two finds replayed around eager calls that rewrite the head of the scratch; four
threads at once, each with its own scratch; OrbFeaturesFinder.find on a list that mixes sizes, channels and host and device images.
Every call, eager or replayed, equals tests/helpers/orb_np.py through test_gpu_orb.check."""
import gc
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_cases as cases  # noqa: E402
import test_gpu_orb as T  # noqa: E402  (check, params_of, CASES / want_of, SENTINEL)
from helpers import orb_np as M  # noqa: E402
from imagestitch_amd import features  # noqa: E402

pytestmark = pytest.mark.gpu
_np = T._np


@pytest.fixture(scope="module", autouse=True)
def release_the_scratch():
    yield
    features.OrbFeaturesFinder.release()


def a_pattern(seed):
    p = np.random.default_rng(seed).integers(-15, 16, (512, 2)).astype(np.int32)
    p[:4] = [[15, 15], [-15, -15], [15, -15], [-15, 15]]
    return p


def outputs(cap, put):
    return [put(np.full((cap, 2), T.SENTINEL, np.float32)), put(np.full((cap, 4), T.SENTINEL, np.float32)), put(np.full((cap, 32), T.SENTINEL, np.uint8)),
            put(np.full((1, 2), T.SENTINEL, np.int32))]


def find(image, p, stream, pattern=None, image_on="device", outputs_on="device", pattern_on="device", wait=True):
    """one isx_orb_find on `stream` with each kind of mat where it is asked to be; the whole output mats as NumPy arrays (wait=False: the
    mats themselves, with nothing waited for)"""
    import torch
    put = {"device": T._dev, "host": np.array}
    with torch.cuda.stream(stream):
        q = T.params_of(p)
        outs = outputs(max(features.capacity(q), 1), put[outputs_on])
        features.orb_find(put[image_on](image), q, *outs, None if pattern is None else put[pattern_on](pattern), 0, stream)
    if not wait:
        return outs
    stream.synchronize()
    return tuple(_np(o) for o in outs)


# ---- a. one thread, one scratch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 2])
def test_a_run_of_calls_on_one_scratch(gpu, streams):
    """large (264 layers), one keypoint, truncated ties, a clean scene (the status word is 0 again), four passes of the final cut, 1 x 1; then
    host mats, a host pattern and a device pattern: the scratch grows, is reused by smaller calls and holds nothing of the call before"""
    import torch
    features.OrbFeaturesFinder.release()                     # the run starts without a scratch and grows it
    ss = [torch.cuda.current_stream()] if streams == 1 else [torch.cuda.Stream(), torch.cuda.Stream()]
    run = [cases.limit_want(n)[:3] + (n,) for n in ("layers-264", "side-63x63", "passes-ties-cut")] + [T.want_of("blobs-1x1") + ("blobs-1x1",)]
    run += [cases.limit_want(n)[:3] + (n,) for n in ("passes-4", "side-1x1")]
    assert [w.status for _, _, w, _ in run] == [0, 0, M.STATUS_TRUNCATED, 0, 0, 0] and [w.count > 0 for _, _, w, _ in run] == [True] * 5 + [False]
    k = 0
    for img, p, want, name in run:
        T.check(find(img, p, ss[k % len(ss)]), want, "%d: %s" % (k, name))
        k += 1
    # the same run twice over with nothing waited for in between: on two streams only the scratch's own fence (scratch.hpp, rule 2) keeps
    # a call from starting in the buffers of the one before
    pending = []
    for img, p, want, name in run + run:
        pending.append((find(img, p, ss[k % len(ss)], wait=False), want, "%d: %s, not waited for" % (k, name)))
        k += 1
    torch.cuda.synchronize()
    for outs, want, what in pending:
        T.check(tuple(_np(o) for o in outs), want, what)
    del pending
    pat = a_pattern(7)
    img, p, _ = T.want_of("blobs-3x1-bgr-cut")
    with_pat = M.find(img, p, pat)
    assert not np.array_equal(with_pat.descriptors, T.want_of("blobs-3x1-bgr-cut")[2].descriptors)
    for kw, want, name in ((dict(image_on="host", outputs_on="host"), cases.limit_want("layers-264")[2], "layers-264"),
                           (dict(image_on="host", outputs_on="host"), cases.limit_want("side-63x63")[2], "side-63x63"),
                           (dict(pattern=pat, pattern_on="host"), with_pat, None), (dict(), T.want_of("blobs-3x1-bgr-cut")[2], None),
                           (dict(pattern=pat, pattern_on="device"), with_pat, None), (dict(image_on="host", outputs_on="host"), T.want_of("blobs-3x1-bgr-cut")[2], None),
                           (dict(), cases.limit_want("passes-ties-cut")[2], "passes-ties-cut")):
        im, pp = (img, p) if name is None else cases.limit_want(name)[:2]
        T.check(find(im, pp, ss[k % len(ss)], **kw), want, "%d: %s %s" % (k, name or "blobs-3x1-bgr-cut", kw))
        k += 1
    torch.cuda.synchronize()


# ---- b. a graph of two finds, replayed around eager calls ---------------------------------------------------------------------------------------
def test_replays_around_eager_calls(gpu):
    """Reserved for the largest image and every parameter set of the test, so that no call grows the scratch (that would free the buffer the
    graph's kernels point into: DESIGN.md §8).  The graph holds find A (default pattern, read from the head of the scratch) and find B (a
    device pattern of the caller's), other parameters, separate outputs.  Between the replays eager calls of the same thread on the same
    stream rewrite the head of the scratch (a host image, a host pattern) and every intermediate buffer."""
    import torch
    big_w, big_h = 400, 300
    PA = M.Params(grid=(2, 1), n_features=300, nlevels=3)
    PB = M.Params(grid=(1, 1), n_features=100)                              # cases.dots under it: ties past the room at both cuts
    PE = M.Params(grid=(1, 1), n_features=80, nlevels=2, fast_threshold=7)
    pat_b, pat_e = a_pattern(8), a_pattern(9)
    a_images = [cases.scene(big_h, big_w, 31), cases.scene(big_h, big_w, 32), np.zeros((big_h, big_w), np.uint8)]
    b_images = [cases.dots(224, 256), cases.scene(224, 256, 33), cases.dots(224, 256, count=100)]
    small = cases.scene(120, 160, 34, 3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    features.OrbFeaturesFinder.release()
    for p in (PA, PB, PE):
        features.orb_reserve(T.params_of(p), big_w, big_h)
    qa, qb = T.params_of(PA), T.params_of(PB)
    with torch.cuda.stream(s):
        d_a, d_b, d_pat = T._dev(a_images[0]), T._dev(b_images[0]), T._dev(pat_b)
        outs_a, outs_b = outputs(features.capacity(qa), T._dev), outputs(features.capacity(qb), T._dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        features.orb_find(d_a, qa, *outs_a, None, 0, s)
        features.orb_find(d_b, qb, *outs_b, d_pat, 0, s)
    eager = [[(small, PE, dict()), (small, PA, dict(image_on="host", outputs_on="host")), (small[:, :, 0].copy(), PB, dict(pattern=pat_e, pattern_on="host"))],
             [(small, PB, dict(image_on="host")), (b_images[0], PE, dict(pattern=pat_e, pattern_on="host", outputs_on="host"))], []]
    statuses = []
    for k, (ia, ib) in enumerate(zip(a_images, b_images)):
        wa, wb = M.find(ia, PA), M.find(ib, PB, pat_b)
        statuses.append(wb.status)
        with torch.cuda.stream(s):
            d_a.copy_(torch.from_numpy(ia).cuda())
            d_b.copy_(torch.from_numpy(ib).cuda())
            for t in outs_a + outs_b:
                t.fill_(T.SENTINEL)
        s.synchronize()
        g.replay()
        torch.cuda.synchronize()
        T.check(tuple(_np(t) for t in outs_a), wa, "replay %d, find A" % k)
        T.check(tuple(_np(t) for t in outs_b), wb, "replay %d, find B" % k)
        for j, (img, p, kw) in enumerate(eager[k]):
            T.check(find(img, p, s, **kw), M.find(img, p, kw.get("pattern")), "eager %d.%d %s" % (k, j, kw))
    assert statuses == [M.STATUS_TRUNCATED, 0, M.STATUS_TRUNCATED]
    del g
    features.OrbFeaturesFinder.release()


# ---- c. four threads -------------------------------------------------------------------------------------------------------------------------
def test_four_threads_each_with_its_own_scratch(gpu):
    """Four threads, each on its own stream with its own pair of (image, parameters), 6 finds each, alternating; everything is kept and
    compared after the join.  Each thread releases what it holds."""
    import torch
    FINDS = 6
    pairs = [("blobs-1x1-cut", "w257"), ("blobs-3x1-bgr-cut", "ties-truncated"), ("blobs-2x2-bgra", "threshold7"), ("passes-2", "64x64")]
    plans = [dict(cases=[cases.limit_want(n)[:3] if n in cases.LIMIT_CASES else T.want_of(n) for n in pair], names=pair, got=[]) for pair in pairs]
    start = threading.Barrier(len(plans))

    def work(errors, plan):
        try:
            try:
                stream = torch.cuda.Stream()
                with torch.cuda.stream(stream):
                    mats = [(T._dev(img), T.params_of(p)) for img, p, _ in plan["cases"]]
                    start.wait(timeout=60)
                    for i in range(FINDS):
                        d_img, q = mats[i % 2]
                        outs = outputs(features.capacity(q), T._dev)
                        features.orb_find(d_img, q, *outs, None, 0, stream)
                        plan["got"].append((i % 2, outs))
                stream.synchronize()
            finally:
                features.OrbFeaturesFinder.release()
        except BaseException as ex:       # noqa: BLE001
            errors.append(ex)

    errors = []
    ts = [threading.Thread(target=work, args=(errors, p)) for p in plans]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "a thread did not finish"
    if errors:
        raise errors[0]
    torch.cuda.synchronize()
    for plan in plans:
        assert len(plan["got"]) == FINDS
        for i, (k, outs) in enumerate(plan["got"]):
            T.check(tuple(_np(o) for o in outs), plan["cases"][k][2], "%s, find %d" % (plan["names"][k], i))


# ---- d. the finder class on a mixed list -----------------------------------------------------------------------------------------------------
def test_the_finder_class_on_a_mixed_list(gpu):
    """sizes that grow and shrink, one channel, three and four, host and device images, an image without a keypoint in the middle"""
    grid, n = (2, 1), 400
    images = [(cases.scene(130, 200, 41), "device"), (cases.scene(224, 256, 42, 3), "host"), (cases.scene(300, 330, 43), "device"), (cases.flat(100, 120), "host"),
              (cases.scene(224, 300, 44, 4), "device"), (cases.scene(100, 150, 45), "host"), (cases.flat(2, 2), "device"), (cases.scene(160, 192, 46, 3), "device")]
    wants = [M.find(img, M.Params(grid=grid, n_features=n)) for img, _ in images]
    assert [w.count > 0 for w in wants] == [True, True, True, False, True, True, False, True]
    f = features.OrbFeaturesFinder(grid, n)
    try:
        feats = f.find([T._dev(img) if where == "device" else img for img, where in images])
        assert len(feats) == len(images)
        for k, (ft, want, (img, where)) in enumerate(zip(feats, wants, images)):
            assert ft.img_idx == k and ft.img_size == (img.shape[1], img.shape[0]) and ft.status == want.status, k
            assert hasattr(ft.keypoints, "cpu") == (where == "device") and hasattr(ft.descriptors, "cpu") == (where == "device"), k
            kp, meta, desc = _np(ft.keypoints), _np(ft.meta), _np(ft.descriptors)
            assert kp.shape == (want.count, 2) and meta.shape == (want.count, 4) and desc.shape == (want.count, 32), k
            assert np.array_equal(kp, want.keypoints) and np.array_equal(meta.view(np.uint32), want.meta.view(np.uint32).reshape(want.count, 4)), k
            assert np.array_equal(desc, want.descriptors), k
    finally:
        f.release()
