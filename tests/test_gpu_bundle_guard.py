"""isx_bundle_adjust_ray writes its outputs and nothing beside them, and a refused call writes nothing at all: every mat lies inside the
guard bands of tests/helpers/guarded.py.  Each refusal of the header - null pointers, one image in a rig, from >= to, a repeated pair, a
pair across two rigs, an index out of range, rig_first not increasing, max_iter outside [1, 1000], a negative or NaN conf_thresh, a NaN eps,
a misaligned mat, another type, too few rows or columns, more than 64 images in a rig, a capturing stream - with host and device mats."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_cases as cases  # noqa: E402
import fuzz_bundle as fz  # noqa: E402
from helpers.guarded import NOTHING, guarded, guarded_like  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402
from imagestitch_amd import adjuster as adj  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_UNSUPPORTED, ERR_SIZE = 1, 2, 3, 6, 7
NAMED = cases.named()


def _case():
    return cases.join([dict(NAMED["camera_without_edge"], max_iter=3), NAMED["max_iter_3"]])      # 7 images, 9 pairs, rig_first [0, 4, 7]


def _mats(c, where, layout, seed=1):
    """Inputs (holding the case) and outputs (random bytes) inside guard bands."""
    n, nrigs = len(c["sizes"]), len(c["rig_first"]) - 1
    ins = dict(counts=guarded_like(c["counts"], where, layout, seed, "counts"), stats=guarded_like(c["stats"], where, layout, seed + 1, "stats"),
               conf=guarded_like(c["conf"], where, layout, seed + 2, "conf"), est=guarded_like(c["est_rig_stats"], where, layout, seed + 3, "est_rig_stats"),
               cin=guarded_like(c["cameras_in"], where, layout, seed + 4, "cameras_in"))
    for i, k in enumerate(c["keypoints"]):
        ins["kp%d" % i] = guarded_like(k, where, layout, seed + 10 + i, "keypoints %d" % i)
    for p, (m, k) in enumerate(zip(c["matches"], c["masks"])):
        ins["mt%d" % p] = guarded_like(m, where, layout, seed + 30 + p, "matches %d" % p)
        ins["mk%d" % p] = guarded_like(k, where, layout, seed + 60 + p, "inlier_masks %d" % p)
    outs = dict(cameras_out=guarded((n, 16), np.float64, where, layout, seed + 5, "cameras_out"), kr32_out=guarded((n, 18), np.float32, where, layout, seed + 6, "kr32_out"),
                rig_stats_out=guarded((nrigs, 8), np.int32, where, layout, seed + 7, "rig_stats_out"),
                rig_err_out=guarded((nrigs, 2), np.float64, where, layout, seed + 8, "rig_err_out"))
    return ins, outs


def _call(c, ins, outs, stream=None, **over):
    n, npairs = len(c["sizes"]), len(c["pairs"])
    a = dict(img_sizes=c["sizes"], keypoints=[ins["kp%d" % i].view for i in range(n)], pairs=c["pairs"], matches=[ins["mt%d" % p].view for p in range(npairs)],
             masks=[ins["mk%d" % p].view for p in range(npairs)], counts=ins["counts"].view, stats=ins["stats"].view, conf=ins["conf"].view,
             est_rig_stats=ins["est"].view, cameras_in=ins["cin"].view, cameras_out=outs["cameras_out"].view, kr32_out=outs["kr32_out"].view,
             rig_stats_out=outs["rig_stats_out"].view, rig_err_out=outs["rig_err_out"].view, rig_first=c["rig_first"], conf_thresh=c["conf_thresh"],
             max_iter=c["max_iter"], stream=stream)
    a.update(over)
    return adj.bundle_adjust_ray(**a)


def _untouched(ins, outs):
    import torch
    torch.cuda.synchronize()
    for g in list(ins.values()) + list(outs.values()):
        g.check(written=NOTHING)


@pytest.mark.parametrize("where,layout", [("device", "aligned"), ("device", "odd"), ("host", "odd"), ("host", "aligned")])
def test_a_call_writes_its_outputs_and_nothing_beside_them(gpu, where, layout):
    import torch
    c = _case()
    ins, outs = _mats(c, where, layout)
    assert _call(c, ins, outs) == (2, 1)
    torch.cuda.synchronize()
    for g in ins.values():
        g.check(written=NOTHING)
    for g in outs.values():
        g.check()
    want = fz.run_model(c)
    for g, w in zip(outs.values(), want):
        assert fz.same(g.get(), w) and not np.isnan(w.astype(np.float64)).any(), g.name


def _refusals(c):
    """(name, status, overrides of _call's arguments)"""
    n, npairs = len(c["sizes"]), len(c["pairs"])
    p = list(c["pairs"])
    raw = np.zeros(n * 16 * 8 + 16, np.uint8)
    m0 = c["matches"][0]
    swap = lambda lst, k, v: lst[:k] + [v] + lst[k + 1:]      # noqa: E731
    return [
        ("one image in a rig", ERR_INVALID, dict(rig_first=[0, 1, 7])),
        ("from >= to", ERR_INVALID, dict(pairs=swap(p, 3, (p[3][1], p[3][0])))),
        ("from == to", ERR_INVALID, dict(pairs=swap(p, 3, (2, 2)))),
        ("a repeated pair", ERR_INVALID, dict(pairs=swap(p, npairs - 1, p[6]))),
        ("a pair across two rigs", ERR_INVALID, dict(pairs=swap(p, npairs - 1, (3, 4)))),
        ("an index out of range", ERR_INVALID, dict(pairs=swap(p, npairs - 1, (5, n)))),
        ("a negative index", ERR_INVALID, dict(pairs=swap(p, npairs - 1, (-1, 2)))),
        ("rig_first not increasing", ERR_INVALID, dict(rig_first=[0, 4, 2, 7])),
        ("rig_first past the images", ERR_INVALID, dict(rig_first=[0, 4, 8])),
        ("max_iter 0", ERR_INVALID, dict(max_iter=0)),
        ("max_iter 1001", ERR_INVALID, dict(max_iter=1001)),
        ("a negative conf_thresh", ERR_INVALID, dict(conf_thresh=-0.5)),
        ("a NaN conf_thresh", ERR_INVALID, dict(conf_thresh=float("nan"))),
        ("a NaN eps", ERR_INVALID, dict(eps=float("nan"))),
        ("a misaligned cameras_in", ERR_INVALID, dict(cameras_in=np.frombuffer(raw, np.float64, n * 16, 4).reshape(n, 16))),
        ("stats of another type", ERR_TYPE, dict(stats=np.zeros((npairs, 8), np.float32))),
        ("conf of another type", ERR_TYPE, dict(conf=np.zeros((1, npairs), np.float32))),
        ("matches of another type", ERR_TYPE, dict(matches=[m0.astype(np.float32)] + c["matches"][1:])),
        ("a mask of another type", ERR_TYPE, dict(masks=[c["masks"][0].astype(np.int32)] + c["masks"][1:])),
        ("keypoints of another type", ERR_TYPE, dict(keypoints=[c["keypoints"][0].astype(np.float64)] + c["keypoints"][1:])),
        ("keypoints with one column", ERR_SIZE, dict(keypoints=[np.ascontiguousarray(c["keypoints"][0][:, :1])] + c["keypoints"][1:])),
        ("matches with two columns", ERR_SIZE, dict(matches=[np.ascontiguousarray(m0[:, :2])] + c["matches"][1:])),
        ("counts too short", ERR_SIZE, dict(counts=np.zeros((1, npairs - 1), np.int32))),
        ("conf too short", ERR_SIZE, dict(conf=np.zeros((1, npairs - 1)))),
        ("est_rig_stats with one row", ERR_SIZE, dict(est_rig_stats=np.zeros((1, 8), np.int32))),
        ("cameras_in with 15 columns", ERR_SIZE, dict(cameras_in=np.zeros((n, 15)))),
        ("65 images in a rig", ERR_UNSUPPORTED, dict(img_sizes=[(640, 480)] * 67, rig_first=[0, 65, 67], pairs=[], matches=[], masks=[],
                                                    keypoints=[np.zeros((1, 2), np.float32)] * 67, cameras_in=np.zeros((67, 16)))),
    ]


@pytest.mark.parametrize("where", ["device", "host"])
def test_refusals_write_not_one_byte(gpu, where):
    c = _case()
    ins, outs = _mats(c, where, "aligned", 20)
    n = len(c["sizes"])
    for name, code, over in _refusals(c):
        if "65 images" in name:      # outputs large enough, so that the rig's size alone is what is refused
            big = dict(cameras_out=guarded((67, 16), np.float64, where, "aligned", 31), kr32_out=guarded((67, 18), np.float32, where, "aligned", 32),
                       rig_stats_out=guarded((2, 8), np.int32, where, "aligned", 33), rig_err_out=guarded((2, 2), np.float64, where, "aligned", 34))
            with pytest.raises(_lib.IsxError) as e:
                _call(c, ins, big, **over)
            assert e.value.code == code, (name, e.value)
            _untouched(ins, big)
            continue
        with pytest.raises(_lib.IsxError) as e:
            _call(c, ins, outs, **over)
        assert e.value.code == code, (name, e.value)
        _untouched(ins, outs)
    # an output too small, of another type: the other outputs stay untouched as well
    for key, shape, dtype, code in (("cameras_out", (n, 15), np.float64, ERR_SIZE), ("kr32_out", (n - 1, 18), np.float32, ERR_SIZE),
                                    ("rig_stats_out", (1, 8), np.int32, ERR_SIZE), ("rig_err_out", (2, 2), np.float32, ERR_TYPE),
                                    ("rig_err_out", (2, 1), np.float64, ERR_SIZE), ("kr32_out", (n, 18), np.int32, ERR_TYPE)):
        g = guarded(shape, dtype, where, "aligned", 40, key)
        with pytest.raises(_lib.IsxError) as e:
            _call(c, ins, outs, **{key: g.view})
        assert e.value.code == code, (key, shape, e.value)
        _untouched(ins, outs)
        g.check(written=NOTHING)


def test_null_pointers_are_refused(gpu):
    c = _case()
    ins, outs = _mats(c, "device", "aligned", 50)
    lib = _lib.load()
    n, npairs = len(c["sizes"]), len(c["pairs"])
    sizes = (C.c_int * (2 * n))(*[int(v) for s in c["sizes"] for v in s])
    pij = (C.c_int * (2 * npairs))(*[int(v) for p in c["pairs"] for v in p])
    first = (C.c_int * 3)(*c["rig_first"])
    kps = (_lib.IsxMat * n)(*[_lib.as_mat(ins["kp%d" % i].view) for i in range(n)])
    mts = (_lib.IsxMat * npairs)(*[_lib.as_mat(ins["mt%d" % p].view) for p in range(npairs)])
    mks = (_lib.IsxMat * npairs)(*[_lib.as_mat(ins["mk%d" % p].view) for p in range(npairs)])
    one = {k: C.byref(_lib.as_mat(g.view)) for k, g in list(ins.items()) + list(outs.items()) if not k[:2] in ("kp", "mt", "mk")}
    full = [n, sizes, kps, npairs, pij, mts, mks, one["counts"], one["stats"], one["conf"], 2, first, one["est"], one["cin"], C.c_double(1.0), 3,
            C.c_double(2.0 ** -52), one["cameras_out"], one["kr32_out"], one["rig_stats_out"], one["rig_err_out"], None, 0, C.c_void_p(0)]
    for at in (1, 2, 4, 5, 6, 7, 8, 9, 12, 13, 17, 18, 19, 20):
        args = list(full)
        args[at] = None
        assert lib.isx_bundle_adjust_ray(*args) == ERR_INVALID, at
        _untouched(ins, outs)
    args = list(full)
    args[11] = None                      # two rigs without rig_first
    assert lib.isx_bundle_adjust_ray(*args) == ERR_INVALID
    _untouched(ins, outs)
    assert lib.isx_bundle_adjust_ray(*full) == 0


def test_a_capturing_stream_is_refused_with_nothing_enqueued(gpu):
    import torch
    c = _case()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ins, outs = _mats(c, "device", "aligned", 60)
        x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(_lib.IsxError) as e:
            _call(c, ins, outs, stream=s)
        assert e.value.code == ERR_STATE and "captur" in e.value.msg
    torch.cuda.synchronize()
    assert float(x[0]) == 0.0                                      # captured, not run; the capture is intact
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    _untouched(ins, outs)
    assert _call(c, ins, outs, stream=s) == (2, 1)                 # the same stream works after the capture
    s.synchronize()
    want = fz.run_model(c)
    assert all(fz.same(g_.get(), w) for g_, w in zip(outs.values(), want))
    adj.release()
