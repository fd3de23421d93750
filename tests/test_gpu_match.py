"""The features matcher on the GPU (isx_match_features, imagestitch_amd/matcher.py) against the NumPy model of tests/helpers/match_np.py,
np.array_equal throughout: matches, counts, points and knn over shapes built from the kernel's tiling constants, the degenerate shapes, the
float32 rounding cases, duplicate train rows, many pairs in one call, host and device layouts inside guard bands, every error status, a
capturing stream, long-lived use on a non-default stream, and the C++ mirror."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_cases as cases  # noqa: E402
from helpers import guarded  # noqa: E402
from helpers import match_np as M  # noqa: E402
from imagestitch_amd import matcher  # noqa: E402

pytestmark = pytest.mark.gpu
Q, T, CHUNK = matcher.QUERY_BLOCK, matcher.TRAIN_TILE, matcher.TRAIN_CHUNK
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_UNSUPPORTED, ERR_SIZE = 1, 2, 3, 6, 7
SENTINEL = -7777


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _sync():
    import torch
    torch.cuda.synchronize()


def run_raw(descs, pairs, conf, keypoints=None, sizes=None, device=True, knn=True, stream=None):
    """isx_match_features on dense mats (device tensors or host arrays) pre-filled with a sentinel; returns (records, info): per pair a dict of
    count, matches, points, knn as NumPy arrays - the whole mats, rows past the count included."""
    put = _dev if device else (lambda a: np.array(a))
    cap = [descs[i].shape[0] + descs[j].shape[0] for i, j in pairs]
    ms = [put(np.full((n, 3), SENTINEL, np.int32)) for n in cap]
    ps = [put(np.full((n, 4), SENTINEL, np.float32)) for n in cap] if keypoints is not None else None
    ks = [put(np.full((descs[p[d]].shape[0], 4), SENTINEL, np.int32)) for p in pairs for d in range(2)] if knn else None
    cnt = put(np.full((1, max(len(pairs), 1)), SENTINEL, np.int32))
    info = matcher.match_features([put(d) for d in descs], pairs, conf, ms, cnt, None if keypoints is None else [put(k) for k in keypoints], sizes, ps, ks,
                                  0, stream)
    _sync()
    out = []
    for k in range(len(pairs)):
        out.append(dict(count=int(_np(cnt)[0, k]), matches=_np(ms[k]), points=_np(ps[k]) if ps else None,
                        knn=(_np(ks[2 * k]), _np(ks[2 * k + 1])) if ks else None))
    return out, info


def check_against_model(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want)):
        c = w["count"]
        assert g["count"] == c, (what, k, g["count"], c)
        assert np.array_equal(g["matches"][:c], w["matches"]), (what, k)
        assert (g["matches"][c:] == SENTINEL).all(), (what, k, "rows past the count were written")
        if g["points"] is not None:
            assert np.array_equal(g["points"][:c], w["points"]), (what, k)
            assert (g["points"][c:] == SENTINEL).all(), (what, k)
        if g["knn"] is not None:
            for d in range(2):
                if w["skipped"]:
                    assert (g["knn"][d] == SENTINEL).all(), (what, k, d)
                else:
                    assert np.array_equal(g["knn"][d], w["knn"][d]), (what, k, d)


SHAPES = [(nf, nt) for nf in (Q - 1, Q, Q + 1) for nt in (T - 1, T, T + 1)] + [(2 * Q + 1, 2 * T + 1), (Q + 3, CHUNK - 1), (Q - 3, CHUNK), (Q + 5, CHUNK + 1),
                                                                                  (CHUNK + 1, 2 * CHUNK + 1)]


@pytest.mark.parametrize("n_from,n_to", SHAPES)
def test_tile_and_chunk_shapes(gpu, n_from, n_to):
    a, b, planted = cases.planted_pair(1000 * n_from + n_to, n_from, n_to)
    assert [t for _, _, t in planted["mutual"]] == list(range(17))
    kps, sizes = cases.keypoints_for(n_from + n_to, [n_from, n_to])
    want = M.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
    assert min(want[0]["kinds"]) >= 1
    for device in (True, False):
        got, info = run_raw([a, b], [(0, 1)], 0.3, kps, sizes, device=device)
        check_against_model(got, want, "device" if device else "host")
        assert info[0] == 1 and info[1] == (3 if device else 2)


@pytest.mark.parametrize("name", sorted(cases.degenerate_cases()))
def test_degenerate_shapes(gpu, name):
    descs, pairs, conf = cases.degenerate_cases()[name]
    kps, sizes = cases.keypoints_for(3, [d.shape[0] for d in descs])
    want = M.match_model(descs, pairs, conf, kps, sizes)
    for device in (True, False):
        got, info = run_raw(descs, pairs, conf, kps, sizes, device=device)
        check_against_model(got, want, name)
        assert info[0] == (0 if want[0]["skipped"] else 1)


def test_float32_rounding_cases(gpu):
    """The twelve (7j, 20j) at match_conf = 0.65, which float32 accepts and exact arithmetic rejects, in one call (cases.rounding_cases says
    why not in one pair); at 0.66 none is accepted."""
    descs, pairs = cases.rounding_cases()
    want = M.match_model(descs, pairs, cases.ROUNDING_CONF)
    assert [w["count"] for w in want] == [1] * 12
    got, info = run_raw(descs, pairs, cases.ROUNDING_CONF)
    check_against_model(got, want)
    for (d0, d1), g in zip(cases.ROUNDING, got):
        assert sorted(g["knn"][0][0, [1, 3]]) == [d0, d1] and g["matches"][0, 2] == d0
    got, _ = run_raw(descs, pairs, 0.66)
    assert [g["count"] for g in got] == [0] * 12


def test_duplicate_train_rows_and_tie_independence(gpu):
    a, b, _ = cases.planted_pair(3, Q + 9, T + 40, "duplicates")
    b[T + 1] = b[2]                                               # a duplicate across the tile boundary as well
    want = M.match_model([a, b], [(0, 1)], 0.3)
    got, _ = run_raw([a, b], [(0, 1)], 0.3)
    check_against_model(got, want)
    k12 = got[0]["knn"][0]
    ties = np.flatnonzero(k12[:, 1] == k12[:, 3])
    assert len(ties) > 0 and (k12[ties, 0] < k12[ties, 2]).all()  # the lower row first
    perm = np.random.default_rng(5).permutation(b.shape[0])
    got2, _ = run_raw([a, b[perm]], [(0, 1)], 0.3)
    m, m2 = got[0]["matches"][: got[0]["count"]], got2[0]["matches"][: got2[0]["count"]].copy()
    assert got2[0]["count"] == got[0]["count"]
    m2[:, 1] = perm[m2[:, 1]]
    n12 = int(M.accepted(want[0]["knn"][0], 0.3).sum())
    assert np.array_equal(m2[:n12], m[:n12]) and sorted(map(tuple, m2[n12:])) == sorted(map(tuple, m[n12:]))


def test_many_pairs_in_one_call(gpu):
    rows = [Q - 2, Q + 1, Q // 2 + 3, Q + 17, 2 * Q - 5]
    rng = np.random.default_rng(77)
    import fuzz_match
    all_pairs = M.near_pairs(rows)
    assert len(all_pairs) == 10
    descs, _ = fuzz_match.build(rng, rows, all_pairs)
    kps, sizes = cases.keypoints_for(5, rows)
    want = M.match_model(descs, all_pairs, 0.3, kps, sizes)
    assert all(min(w["kinds"]) >= 1 for w in want)
    got, info10 = run_raw(descs, all_pairs, 0.3, kps, sizes)
    check_against_model(got, want)
    launches = set()
    for k, (i, j) in enumerate(all_pairs):                        # the same pair matched alone
        alone, info1 = run_raw([descs[i], descs[j]], [(0, 1)], 0.3, [kps[i], kps[j]], [sizes[i], sizes[j]])
        launches.add(info1[1])
        for key in ("count", "matches", "points"):
            assert np.array_equal(alone[0][key], got[k][key]), (k, key)
        assert all(np.array_equal(alone[0]["knn"][d], got[k]["knn"][d]) for d in range(2))
    assert info10 == (10, 3) and launches == {3}                  # three launches for one pair and for ten
    mask = np.ones((5, 5), np.uint8)
    for i, j in ((0, 2), (1, 4), (3, 4)):
        mask[i, j] = 0
    fm = gpu.FeaturesMatcher(0.3)
    for place in (_dev, np.array):
        recs = fm.match([place(d) for d in descs], [place(k) for k in kps], sizes, mask=mask, knn=True)
        kept = M.near_pairs(rows, mask)
        assert len(kept) == 7 and [(r.src_img_idx, r.dst_img_idx) for r in recs] == kept and fm.last_info[0] == 7
        for r in recs:
            w = want[all_pairs.index((r.src_img_idx, r.dst_img_idx))]
            assert np.array_equal(_np(r.matches), w["matches"]) and np.array_equal(_np(r.src_points), w["points"][:, :2])
            assert np.array_equal(_np(r.dst_points), w["points"][:, 2:]) and all(np.array_equal(_np(r.knn[d]), w["knn"][d]) for d in range(2))
    assert fm.match([descs[0], np.zeros((0, 32), np.uint8)]) == []


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("layout", guarded.LAYOUTS)
def test_layouts_inside_guard_bands(gpu, where, layout):
    """Descriptors with an odd data pointer and a step of 33 / 40 bytes (and the guarded layouts), padded outputs: the inputs and every byte
    outside the written rows - the rows from counts[p] on included - are untouched."""
    rows = [Q + 1, 37, T + 2]
    pairs = [(0, 1), (0, 2), (1, 2)]
    import fuzz_match
    descs, _ = fuzz_match.build(np.random.default_rng(9), rows, pairs)
    kps, sizes = cases.keypoints_for(9, rows)
    want = M.match_model(descs, pairs, 0.3, kps, sizes)
    rng = np.random.default_rng(1)
    placed = [fuzz_match._place(rng, d, where == "device", True) for d in descs[:2]]      # odd pointer, step 33 or 40
    g_d = guarded.guarded_like(descs[2], where, layout, 21, "descriptors 2")
    d_in = [placed[0][0], placed[1][0], g_d.view]
    before = [p[1]() for p in placed]
    g_k = [guarded.guarded_like(k, where, layout, 30 + i, "keypoints %d" % i) for i, k in enumerate(kps)]
    cap = [rows[i] + rows[j] for i, j in pairs]
    g_m = [guarded.guarded((n, 3), np.int32, where, layout, 40 + i, "matches %d" % i) for i, n in enumerate(cap)]
    g_p = [guarded.guarded((n, 4), np.float32, where, layout, 50 + i, "points %d" % i) for i, n in enumerate(cap)]
    g_n = [guarded.guarded((rows[p[d]], 4), np.int32, where, layout, 60 + 2 * i + d, "knn %d" % (2 * i + d)) for i, p in enumerate(pairs) for d in range(2)]
    g_c = guarded.guarded((1, 3), np.int32, where, layout, 70, "counts")
    matcher.match_features(d_in, pairs, 0.3, [g.view for g in g_m], g_c.view, [g.view for g in g_k], sizes, [g.view for g in g_p], [g.view for g in g_n])
    _sync()
    g_d.check(written=guarded.NOTHING)
    assert all(np.array_equal(p[1](), b) for p, b in zip(placed, before))
    for g in g_k:
        g.check(written=guarded.NOTHING)
    g_c.check()
    assert np.array_equal(g_c.get()[0], [w["count"] for w in want])
    for k, w in enumerate(want):
        c = w["count"]
        for g, ref in ((g_m[k], w["matches"]), (g_p[k], w["points"])):
            may = np.zeros(g.shape, bool)
            may[:c] = True
            g.check(written=may)
            assert np.array_equal(g.get()[:c], ref), k
        for d in range(2):
            g_n[2 * k + d].check()
            assert np.array_equal(g_n[2 * k + d].get(), w["knn"][d])


def _expect(code, fn):
    with pytest.raises(matcher._lib.IsxError) as e:
        fn()
    assert e.value.code == code, (e.value.code, e.value.msg)


def test_errors_leave_the_outputs_untouched(gpu):
    import ctypes as C
    a, b, _ = cases.planted_pair(1, 24, 30)
    kps, sizes = cases.keypoints_for(1, [24, 30])
    d = [_dev(a), _dev(b)]
    k = [_dev(kps[0]), _dev(kps[1])]
    m, p, c = _dev(np.full((54, 3), SENTINEL, np.int32)), _dev(np.full((54, 4), SENTINEL, np.float32)), _dev(np.full((1, 1), SENTINEL, np.int32))
    kn = [_dev(np.full((24, 4), SENTINEL, np.int32)), _dev(np.full((30, 4), SENTINEL, np.int32))]

    def call(descs=d, pairs=((0, 1),), conf=0.3, ms=None, cnt=None, kp=k, sz=sizes, ps=None, ks=None):
        return lambda: matcher.match_features(descs, list(pairs), conf, [m] if ms is None else ms, c if cnt is None else cnt, kp, sz,
                                              [p] if ps is None else ps, kn if ks is None else ks)
    _expect(ERR_INVALID, call(pairs=((1, 0),)))
    _expect(ERR_INVALID, call(pairs=((0, 0),)))
    _expect(ERR_INVALID, call(pairs=((0, 2),)))
    _expect(ERR_INVALID, call(pairs=((-1, 1),)))
    for conf in (-0.01, 1.0, 1.5, float("nan"), float("inf")):
        _expect(ERR_INVALID, call(conf=conf))
    _expect(ERR_INVALID, call(sz=None))                                        # keypoints without image sizes
    _expect(ERR_TYPE, call(descs=[_dev(a.astype(np.float32)), d[1]]))
    _expect(ERR_TYPE, call(ms=[_dev(np.zeros((54, 3), np.float32))]))
    _expect(ERR_TYPE, call(ps=[_dev(np.zeros((54, 4), np.int32))]))
    _expect(ERR_TYPE, call(cnt=_dev(np.zeros((1, 1), np.float32))))
    _expect(ERR_TYPE, call(ks=[kn[0], _dev(np.zeros((30, 4), np.float32))]))
    _expect(ERR_TYPE, call(kp=[k[0], _dev(kps[1].astype(np.int32))]))
    _expect(ERR_UNSUPPORTED, call(descs=[_dev(np.zeros((24, 64), np.uint8)), d[1]]))
    _expect(ERR_UNSUPPORTED, call(descs=[_dev(np.zeros((24, 16), np.uint8)), d[1]]))
    _expect(ERR_SIZE, call(ms=[_dev(np.zeros((53, 3), np.int32))]))
    _expect(ERR_SIZE, call(ms=[_dev(np.zeros((54, 2), np.int32))]))
    _expect(ERR_SIZE, call(ps=[_dev(np.zeros((54, 3), np.float32))]))
    _expect(ERR_SIZE, call(ks=[_dev(np.zeros((23, 4), np.int32)), kn[1]]))
    _expect(ERR_SIZE, call(pairs=((0, 1), (0, 1)), ms=[m, m], ps=[p, p], ks=kn + kn))      # counts holds one pair
    _expect(ERR_SIZE, call(kp=[k[0], _dev(kps[1][:29])]))
    # the row limits, on mats that only claim their rows (the checks run before anything is read)
    lib = matcher._lib.load()
    IsxMat = matcher._lib.IsxMat

    def claim(rows):
        return IsxMat(d[0].data_ptr(), rows, 32, 0, 32, 0)
    mats_m, one = (IsxMat * 1)(matcher._lib.as_mat(m)), (C.c_int * 2)(0, 1)
    big = (IsxMat * 2)(claim((1 << 20) + 1), claim(8))
    assert lib.isx_match_features(2, big, None, None, 1, one, 0.3, mats_m, None, C.byref(matcher._lib.as_mat(c)), None, None, 0, None) == ERR_UNSUPPORTED
    many = (IsxMat * 5)(*[claim(1 << 20) for _ in range(4)], claim(1))
    assert lib.isx_match_features(5, many, None, None, 1, one, 0.3, mats_m, None, C.byref(matcher._lib.as_mat(c)), None, None, 0, None) == ERR_UNSUPPORTED
    for null in range(4):                                                      # null descriptors, pairs, matches, counts
        args = [2, (IsxMat * 2)(matcher._lib.as_mat(d[0]), matcher._lib.as_mat(d[1])), None, None, 1, one, 0.3, mats_m, None, C.byref(matcher._lib.as_mat(c)),
                None, None, 0, None]
        args[(1, 5, 7, 9)[null]] = None
        assert lib.isx_match_features(*args) == ERR_INVALID, null
    assert lib.isx_match_features(-1, None, None, None, 0, None, 0.3, None, None, None, None, None, 0, None) == ERR_INVALID
    _sync()
    for t in [m, p, c] + kn:
        assert (_np(t) == SENTINEL).all()
    assert np.array_equal(_np(d[0]), a) and np.array_equal(_np(d[1]), b)
    got, _ = run_raw([a, b], [(0, 1)], 0.3, kps, sizes)            # still usable
    check_against_model(got, M.match_model([a, b], [(0, 1)], 0.3, kps, sizes))


def test_a_capturing_stream_is_refused_with_nothing_enqueued(gpu):
    import torch
    a, b, _ = cases.planted_pair(2, 40, 50)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = [_dev(a), _dev(b)]
        m, c = _dev(np.full((90, 3), SENTINEL, np.int32)), _dev(np.full((1, 1), SENTINEL, np.int32))
        x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(gpu.IsxError) as e:
            matcher.match_features(d, [(0, 1)], 0.3, [m], c, stream=s)
        assert e.value.code == ERR_STATE and "captur" in e.value.msg
    torch.cuda.synchronize()
    assert float(x[0]) == 0.0                                      # captured, not run; the capture is intact
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0 and (_np(m) == SENTINEL).all() and (_np(c) == SENTINEL).all()
    matcher.match_features(d, [(0, 1)], 0.3, [m], c, stream=s)     # the same stream works after the capture
    s.synchronize()
    w = M.match_model([a, b], [(0, 1)], 0.3)[0]
    assert int(_np(c)[0, 0]) == w["count"] and np.array_equal(_np(m)[: w["count"]], w["matches"])


def test_long_lived_use_on_a_stream(gpu):
    """A larger problem, then a smaller one, release(), then again, on a non-default stream: the same results every time."""
    import torch
    big = cases.planted_pair(4, 2 * Q + 7, CHUNK + 9)[:2]
    small = cases.planted_pair(5, 31, 29)[:2]
    kb, sb = cases.keypoints_for(4, [x.shape[0] for x in big])
    ks, ss = cases.keypoints_for(5, [x.shape[0] for x in small])
    want_b, want_s = M.match_model(list(big), [(0, 1)], 0.3, kb, sb), M.match_model(list(small), [(0, 1)], 0.3, ks, ss)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for device in (True, False):
            check_against_model(run_raw(list(big), [(0, 1)], 0.3, kb, sb, device=device, stream=s)[0], want_b, "big")
            check_against_model(run_raw(list(small), [(0, 1)], 0.3, ks, ss, device=device, stream=s)[0], want_s, "small")
            gpu.FeaturesMatcher.release()
            check_against_model(run_raw(list(small), [(0, 1)], 0.3, ks, ss, device=device, stream=s)[0], want_s, "small after release")
            check_against_model(run_raw(list(big), [(0, 1)], 0.3, kb, sb, device=device, stream=s)[0], want_b, "big after release")
        fm = gpu.FeaturesMatcher(0.3, stream=s)
        rec = fm.match([_dev(x) for x in big], [_dev(k) for k in kb], sb)[0]
        assert np.array_equal(_np(rec.matches), want_b[0]["matches"]) and np.array_equal(_np(rec.src_points), want_b[0]["points"][:, :2])
    gpu.FeaturesMatcher.release()
    gpu.FeaturesMatcher.release()                                  # twice is fine


def test_cpp_matcher_demo(gpu, tmp_path):
    """tests/cpp/matcher_demo.cpp through isx::FeaturesMatcher (match() and operator() on ImageFeatures), plain g++ against the C-ABI library."""
    lib_dir = os.path.join(ROOT, "imagestitch_amd", "csrc")
    exe = str(tmp_path / "matcher_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "matcher_demo.cpp"), "-o", exe, "-L", lib_dir, "-limagestitch_hip", "-Wl,-rpath," + lib_dir])
    import fuzz_match
    rows = [40, 0, 55, 33]
    pairs = M.near_pairs(rows)
    descs, _ = fuzz_match.build(np.random.default_rng(12), rows, pairs)
    kps, sizes = cases.keypoints_for(12, rows)
    want = M.match_model(descs, pairs, 0.3, kps, sizes)
    d = tmp_path / "in"
    d.mkdir()
    args = [exe, str(d), "0.3"]
    for k in range(4):
        descs[k].tofile(str(d / ("desc%d.bin" % k)))
        kps[k].tofile(str(d / ("kp%d.bin" % k)))
        args += [str(rows[k]), str(sizes[k][0]), str(sizes[k][1])]
    out = subprocess.check_output(args, text=True, timeout=300)
    lines = out.split("\n")
    assert [ln for ln in lines if ln.startswith("pair")] == ["pair %d %d %d" % (i, j, w["count"]) for (i, j), w in zip(pairs, want)], out
    assert [ln for ln in lines if ln.startswith("entry")] == ["entry %d %d %d" % (i, j, w["count"]) for (i, j), w in zip(pairs, want)], out
    assert "launches 2" in lines, out                              # host mats: packed on the host, so search and finalise only
    for (i, j), w in zip(pairs, want):
        assert np.array_equal(np.fromfile(str(d / ("matches_%d_%d.bin" % (i, j))), np.int32).reshape(-1, 3), w["matches"])
        assert np.array_equal(np.fromfile(str(d / ("points_%d_%d.bin" % (i, j))), np.float32).reshape(-1, 4), w["points"])
