"""The float features matcher on the GPU (isx_match_features_f32, imagestitch_amd/matcher.py) against the NumPy model of
tests/helpers/match_f32_np.py, np.array_equal throughout: the hand case, the float32 rounding table, rows whose squared distance depends on
the order of the sum, special values, every width either side of the padding, shapes on the tiling constants, 28 pairs in one call, host
and device layouts inside guard bands, knn and points on and off, every error status and a capturing stream."""
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_f32_cases as cases  # noqa: E402
from helpers import guarded  # noqa: E402
from helpers import match_f32_np as MF  # noqa: E402
from imagestitch_amd import matcher  # noqa: E402

pytestmark = pytest.mark.gpu
Q, T, CHUNK = matcher.QUERY_BLOCK, matcher.F32_TRAIN_TILE, matcher.TRAIN_CHUNK
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_UNSUPPORTED, ERR_SIZE = 1, 2, 3, 6, 7
SENTINEL = -7777
F32 = np.float32


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _strided(a, device):
    """`a` as a view with padded rows (a step of cols * 4 + 4 .. 12 bytes) behind a 4-byte lead, on the host or the device."""
    import fuzz_match
    return fuzz_match._place(np.random.default_rng(a.shape[0]), a, device, True)[0]


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _sync():
    import torch
    torch.cuda.synchronize()


def run_raw(descs, pairs, conf, keypoints=None, sizes=None, device=True, knn=True, stream=None, strided=False):
    """isx_match_features_f32 on mats (device tensors or host arrays, dense or strided) pre-filled with a sentinel; returns (records, info):
    per pair a dict of count, matches, points, knn as NumPy arrays - the whole mats, rows past the count included."""
    put = (lambda a: _strided(np.asarray(a), device)) if strided else (_dev if device else (lambda a: np.array(a)))
    cap = [descs[i].shape[0] + descs[j].shape[0] for i, j in pairs]
    ms = [put(np.full((n, 3), SENTINEL, np.int32)) for n in cap]
    ps = [put(np.full((n, 4), SENTINEL, np.float32)) for n in cap] if keypoints is not None else None
    ks = [put(np.full((descs[p[d]].shape[0], 4), SENTINEL, np.int32)) for p in pairs for d in range(2)] if knn else None
    cnt = (_dev if device else np.array)(np.full((1, max(len(pairs), 1)), SENTINEL, np.int32))
    info = matcher.match_features_f32([put(d) for d in descs], pairs, conf, ms, cnt, None if keypoints is None else [put(k) for k in keypoints], sizes, ps,
                                      ks, 0, stream)
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


PLACES = [(True, False), (True, True), (False, False), (False, True)]      # (device, strided)


def all_places(descs, pairs, conf, want, kps=None, sizes=None, what=""):
    """The case through device and host mats, contiguous and strided; returns the infos."""
    infos = []
    for device, strided in PLACES:
        got, info = run_raw(descs, pairs, conf, kps, sizes, device=device, strided=strided)
        check_against_model(got, want, (what, device, strided))
        infos.append(info)
    return infos


def test_hand_case(gpu):
    a, b, want = cases.hand_case()
    kps, sizes = cases.keypoints_for(40, [40, 40])
    model = MF.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
    assert np.array_equal(model[0]["matches"], want)
    infos = all_places([a, b], [(0, 1)], 0.3, model, kps, sizes)
    assert infos == [(1, 3), (1, 3), (1, 2), (1, 2)]                 # host mats are packed on the host: search and finalise only


def test_float32_rounding_table(gpu):
    descs, pairs = cases.rounding_cases()
    want = MF.match_model(descs, pairs, cases.ROUNDING_CONF)
    assert [w["count"] for w in want] == [1] * 12
    all_places(descs, pairs, cases.ROUNDING_CONF, want)
    got, _ = run_raw(descs, pairs, 0.66)
    assert [g["count"] for g in got] == [0] * 12


@pytest.mark.parametrize("cols", [64, 128])
def test_the_sum_runs_in_the_stated_order(gpu, cols):
    """Rows for which a reversed sum, four partial sums or an FMA each change which train row is nearest (tests/test_match_f32_model.py
    asserts that they do): the library's knn names the row the stated order names."""
    a, b, _ = cases.order_pair(cols)
    want = MF.match_model([a, b], [(0, 1)], 0.3)
    assert list(want[0]["knn"][0][0, [0, 2]]) == [1, 0]
    all_places([a, b], [(0, 1)], 0.3, want)


@pytest.mark.parametrize("name", sorted(cases.special_cases()))
def test_special_values(gpu, name):
    descs, pairs, conf = cases.special_cases()[name]
    all_places(descs, pairs, conf, MF.match_model(descs, pairs, conf), what=name)


@pytest.mark.parametrize("cols", cases.WIDTHS)
def test_widths(gpu, cols):
    a, b, planted = cases.planted_pair(100 + cols, 20, 23, cols)
    kps, sizes = cases.keypoints_for(cols, [20, 23])
    want = MF.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
    cases.check_planted(want[0], planted)
    all_places([a, b], [(0, 1)], 0.3, want, kps, sizes, cols)
    a2, b2, _ = cases.planted_pair(200 + cols, Q + 3, 2 * T + 1, cols, "cloud")      # rounding-sensitive distances, ratios near 1
    all_places([a2, b2], [(0, 1)], 0.5, MF.match_model([a2, b2], [(0, 1)], 0.5), what=(cols, "cloud"))


@pytest.mark.parametrize("n_from,n_to", cases.shapes())
def test_tile_and_chunk_shapes(gpu, n_from, n_to):
    for cols, filler in ((24, "isolated"), (100, "cloud")):
        a, b, planted = cases.planted_pair(1000 * n_from + n_to + cols, n_from, n_to, cols, filler)
        kps, sizes = cases.keypoints_for(n_from + n_to, [n_from, n_to])
        want = MF.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
        cases.check_planted(want[0], planted)
        assert all_places([a, b], [(0, 1)], 0.3, want, kps, sizes, cols) == [(1, 3), (1, 3), (1, 2), (1, 2)]


@pytest.mark.parametrize("name", sorted(cases.degenerate_cases()))
def test_degenerate_shapes(gpu, name):
    descs, pairs, conf = cases.degenerate_cases()[name]
    kps, sizes = cases.keypoints_for(3, [d.shape[0] for d in descs])
    want = MF.match_model(descs, pairs, conf, kps, sizes)
    for info in all_places(descs, pairs, conf, want, kps, sizes, name):
        assert info[0] == sum(not w["skipped"] for w in want)


def test_knn_and_points_on_and_off(gpu):
    a, b, _ = cases.planted_pair(8, Q + 2, T + 5, 31)
    kps, sizes = cases.keypoints_for(8, [Q + 2, T + 5])
    want = MF.match_model([a, b], [(0, 1)], 0.3, kps, sizes)
    for device in (True, False):
        for with_kp in (True, False):
            for knn in (True, False):
                got, _ = run_raw([a, b], [(0, 1)], 0.3, kps if with_kp else None, sizes if with_kp else None, device=device, knn=knn)
                assert (got[0]["points"] is None) == (not with_kp) and (got[0]["knn"] is None) == (not knn)
                check_against_model(got, want, (device, with_kp, knn))


def test_28_pairs_of_8_images_in_one_call(gpu):
    import fuzz_match_f32
    rows = [Q - 2, Q + 1, T + 3, 2 * T - 1, 61, Q // 2 + 3, 90, 77]
    all_pairs = MF.near_pairs(rows)
    assert len(all_pairs) == 28
    descs, _ = fuzz_match_f32.build(np.random.default_rng(77), rows, all_pairs, 40)
    kps, sizes = cases.keypoints_for(5, rows)
    want = MF.match_model(descs, all_pairs, 0.3, kps, sizes)
    assert all(min(w["kinds"]) >= 1 for w in want)
    got, info28 = run_raw(descs, all_pairs, 0.3, kps, sizes)
    check_against_model(got, want)
    launches = set()
    for k, (i, j) in enumerate(all_pairs):                        # the same pair matched alone: the same bytes
        alone, info1 = run_raw([descs[i], descs[j]], [(0, 1)], 0.3, [kps[i], kps[j]], [sizes[i], sizes[j]])
        launches.add(info1[1])
        for key in ("count", "matches", "points"):
            assert np.array_equal(alone[0][key], got[k][key]), (k, key)
        assert all(np.array_equal(alone[0]["knn"][d], got[k]["knn"][d]) for d in range(2))
    assert info28 == (28, 3) and launches == {3}


def test_the_classes_pick_the_entry_by_dtype(gpu):
    import fuzz_match_f32
    rows = [40, 0, 55, 33]
    pairs = MF.near_pairs(rows)
    descs, _ = fuzz_match_f32.build(np.random.default_rng(12), rows, pairs, 64)
    kps, sizes = cases.keypoints_for(12, rows)
    want = MF.match_model(descs, pairs, 0.3, kps, sizes)
    fm = gpu.FeaturesMatcher(0.3)
    for place in (_dev, np.array):
        recs = fm.match([place(d) for d in descs], [place(k) for k in kps], sizes, knn=True)
        assert [(r.src_img_idx, r.dst_img_idx) for r in recs] == pairs and fm.last_info[0] == 3
        for r, w in zip(recs, want):
            assert np.array_equal(_np(r.matches), w["matches"]) and np.array_equal(_np(r.src_points), w["points"][:, :2])
            assert all(np.array_equal(_np(r.knn[d]), w["knn"][d]) for d in range(2))
            assert r.float_distances and np.array_equal(_np(r.distances), MF.from_bits(w["matches"][:, 2]))
            dual = r.dual()
            assert np.array_equal(dual.matches, w["matches"][:, [1, 0, 2]]) and np.array_equal(dual.distances, _np(r.distances))
    # the Hamming route is untouched and its distances are the integer column converted
    import fuzz_match
    from helpers import match_np as M
    hd, _ = fuzz_match.build(np.random.default_rng(3), [30, 31], [(0, 1)])
    rec = fm.match([_dev(d) for d in hd])[0]
    w = M.match_model(hd, [(0, 1)], 0.3)[0]
    assert np.array_equal(_np(rec.matches), w["matches"]) and np.array_equal(_np(rec.distances), w["matches"][:, 2].astype(F32)) and not rec.float_distances
    with pytest.raises(gpu.IsxError) as e:
        fm.match([_dev(hd[0]), _dev(descs[0])])
    assert e.value.code == ERR_TYPE
    with pytest.raises(gpu.IsxError) as e:                           # the Hamming entry keeps refusing float mats
        matcher.match_features([_dev(descs[0]), _dev(descs[2])], [(0, 1)], 0.3, [_dev(np.zeros((95, 3), np.int32))], _dev(np.zeros((1, 1), np.int32)))
    assert e.value.code == ERR_TYPE


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("layout", guarded.LAYOUTS)
def test_layouts_inside_guard_bands(gpu, where, layout):
    """Guarded inputs and padded outputs: the inputs and every byte outside the written rows - the rows from counts[p] on included - are
    untouched."""
    import fuzz_match_f32
    rows = [Q + 1, 37, T + 2]
    pairs = [(0, 1), (0, 2), (1, 2)]
    descs, _ = fuzz_match_f32.build(np.random.default_rng(9), rows, pairs, 65)
    kps, sizes = cases.keypoints_for(9, rows)
    want = MF.match_model(descs, pairs, 0.3, kps, sizes)
    g_d = [guarded.guarded_like(d, where, layout, 20 + i, "descriptors %d" % i) for i, d in enumerate(descs)]
    g_k = [guarded.guarded_like(k, where, layout, 30 + i, "keypoints %d" % i) for i, k in enumerate(kps)]
    cap = [rows[i] + rows[j] for i, j in pairs]
    g_m = [guarded.guarded((n, 3), np.int32, where, layout, 40 + i, "matches %d" % i) for i, n in enumerate(cap)]
    g_p = [guarded.guarded((n, 4), np.float32, where, layout, 50 + i, "points %d" % i) for i, n in enumerate(cap)]
    g_n = [guarded.guarded((rows[p[d]], 4), np.int32, where, layout, 60 + 2 * i + d, "knn %d" % (2 * i + d)) for i, p in enumerate(pairs) for d in range(2)]
    g_c = guarded.guarded((1, 3), np.int32, where, layout, 70, "counts")
    matcher.match_features_f32([g.view for g in g_d], pairs, 0.3, [g.view for g in g_m], g_c.view, [g.view for g in g_k], sizes, [g.view for g in g_p],
                               [g.view for g in g_n])
    _sync()
    for g in g_d + g_k:
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
    import torch
    a, b, _ = cases.planted_pair(1, 24, 30, 64)
    kps, sizes = cases.keypoints_for(1, [24, 30])
    d = [_dev(a), _dev(b)]
    k = [_dev(kps[0]), _dev(kps[1])]
    m, p, c = _dev(np.full((54, 3), SENTINEL, np.int32)), _dev(np.full((54, 4), SENTINEL, np.float32)), _dev(np.full((1, 1), SENTINEL, np.int32))
    kn = [_dev(np.full((24, 4), SENTINEL, np.int32)), _dev(np.full((30, 4), SENTINEL, np.int32))]

    def call(descs=d, pairs=((0, 1),), conf=0.3, ms=None, cnt=None, kp=k, sz=sizes, ps=None, ks=None):
        return lambda: matcher.match_features_f32(descs, list(pairs), conf, [m] if ms is None else ms, c if cnt is None else cnt, kp, sz,
                                                  [p] if ps is None else ps, kn if ks is None else ks)
    for pr in ((1, 0), (0, 0), (0, 2), (-1, 1)):
        _expect(ERR_INVALID, call(pairs=(pr,)))
    for conf in (-0.01, 1.0, 1.5, float("nan"), float("inf")):
        _expect(ERR_INVALID, call(conf=conf))
    _expect(ERR_INVALID, call(sz=None))                                        # keypoints without image sizes
    _expect(ERR_TYPE, call(descs=[_dev(np.zeros((24, 64), np.uint8)), d[1]]))  # a CV_8UC1 descriptor mat
    _expect(ERR_TYPE, call(descs=[d[0], _dev(np.zeros((30, 32), np.uint8))]))
    _expect(ERR_TYPE, call(ms=[_dev(np.zeros((54, 3), np.float32))]))
    _expect(ERR_TYPE, call(ps=[_dev(np.zeros((54, 4), np.int32))]))
    _expect(ERR_TYPE, call(cnt=_dev(np.zeros((1, 1), np.float32))))
    _expect(ERR_TYPE, call(ks=[kn[0], _dev(np.zeros((30, 4), np.float32))]))
    _expect(ERR_TYPE, call(kp=[k[0], _dev(kps[1].astype(np.int32))]))
    _expect(ERR_UNSUPPORTED, call(descs=[_dev(np.zeros((24, 129), F32)), _dev(np.zeros((30, 129), F32))]))      # cols 129
    _expect(ERR_SIZE, call(descs=[d[0], _dev(np.zeros((30, 63), F32))]))       # differing cols between images
    _expect(ERR_SIZE, call(descs=[_dev(np.zeros((24, 128), F32)), d[1]]))
    _expect(ERR_SIZE, call(ms=[_dev(np.zeros((53, 3), np.int32))]))
    _expect(ERR_SIZE, call(ms=[_dev(np.zeros((54, 2), np.int32))]))
    _expect(ERR_SIZE, call(ps=[_dev(np.zeros((54, 3), np.float32))]))
    _expect(ERR_SIZE, call(ks=[_dev(np.zeros((23, 4), np.int32)), kn[1]]))
    _expect(ERR_SIZE, call(pairs=((0, 1), (0, 1)), ms=[m, m], ps=[p, p], ks=kn + kn))      # counts holds one pair
    _expect(ERR_SIZE, call(kp=[k[0], _dev(kps[1][:29])]))
    # a misaligned step / pointer, and the row limits on mats that only claim their rows (the checks run before anything is read)
    lib = matcher._lib.load()
    IsxMat = matcher._lib.IsxMat
    raw = torch.zeros(64 * 300 + 64, dtype=torch.uint8, device="cuda")

    def claim(rows, cols=64, step=256, lead=0):
        return IsxMat(raw.data_ptr() + lead, rows, cols, matcher._lib.ISX_32FC1, step, 0)
    mats_m, one = (IsxMat * 1)(matcher._lib.as_mat(m)), (C.c_int * 2)(0, 1)
    cm = C.byref(matcher._lib.as_mat(c))
    for bad in ((IsxMat * 2)(claim(24, step=258), claim(30)), (IsxMat * 2)(claim(24), claim(30, lead=2)), (IsxMat * 2)(claim(24, step=252), claim(30))):
        assert lib.isx_match_features_f32(2, bad, None, None, 1, one, 0.3, mats_m, None, cm, None, None, 0, None) == ERR_INVALID
    big = (IsxMat * 2)(claim((1 << 20) + 1), claim(8))
    assert lib.isx_match_features_f32(2, big, None, None, 1, one, 0.3, mats_m, None, cm, None, None, 0, None) == ERR_UNSUPPORTED
    many = (IsxMat * 5)(*[claim(1 << 20) for _ in range(4)], claim(1))
    assert lib.isx_match_features_f32(5, many, None, None, 1, one, 0.3, mats_m, None, cm, None, None, 0, None) == ERR_UNSUPPORTED
    for null in range(4):                                                      # null descriptors, pairs, matches, counts
        args = [2, (IsxMat * 2)(matcher._lib.as_mat(d[0]), matcher._lib.as_mat(d[1])), None, None, 1, one, 0.3, mats_m, None, cm, None, None, 0, None]
        args[(1, 5, 7, 9)[null]] = None
        assert lib.isx_match_features_f32(*args) == ERR_INVALID, null
    assert lib.isx_match_features_f32(-1, None, None, None, 0, None, 0.3, None, None, None, None, None, 0, None) == ERR_INVALID
    _sync()
    for t in [m, p, c] + kn:
        assert (_np(t) == SENTINEL).all()
    assert np.array_equal(_np(d[0]), a) and np.array_equal(_np(d[1]), b)
    got, _ = run_raw([a, b], [(0, 1)], 0.3, kps, sizes)            # still usable
    check_against_model(got, MF.match_model([a, b], [(0, 1)], 0.3, kps, sizes))


def test_a_capturing_stream_is_refused_with_nothing_enqueued(gpu):
    import torch
    a, b, _ = cases.planted_pair(2, 40, 50, 16)
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
            matcher.match_features_f32(d, [(0, 1)], 0.3, [m], c, stream=s)
        assert e.value.code == ERR_STATE and "captur" in e.value.msg
    torch.cuda.synchronize()
    assert float(x[0]) == 0.0                                      # captured, not run; the capture is intact
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0 and (_np(m) == SENTINEL).all() and (_np(c) == SENTINEL).all()
    matcher.match_features_f32(d, [(0, 1)], 0.3, [m], c, stream=s)     # the same stream works after the capture
    s.synchronize()
    w = MF.match_model([a, b], [(0, 1)], 0.3)[0]
    assert int(_np(c)[0, 0]) == w["count"] and np.array_equal(_np(m)[: w["count"]], w["matches"])
    gpu.FeaturesMatcher.release()                                  # the scratch both entries share
