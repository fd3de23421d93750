"""isx_bundle_adjust_reproj and isx_wave_correct write their outputs and nothing beside them, and a refused call writes nothing at all: every
mat lies inside the guard bands of tests/helpers/guarded.py.  For the adjuster every refusal of the Ray entry (tests/test_gpu_bundle_guard.py
lists them: null pointers, one image in a rig, from >= to, a repeated pair, a pair across two rigs, an index out of range, rig_first not
increasing, max_iter, conf_thresh, eps, a misaligned mat, another type, too few rows or columns, more than 64 images in a rig) and its own -
refine_flags outside [0, 31]; for the wave correction null pointers, no image, rig_first, kind, type, size and alignment; a capturing stream
for both."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_reproj_cases as cases  # noqa: E402
import fuzz_bundle_reproj as fz  # noqa: E402
import test_gpu_bundle_guard as ray  # noqa: E402  (its mats in guard bands and its table of refusals)
from helpers import bundle_reproj_np as rp  # noqa: E402
from helpers.guarded import NOTHING, guarded, guarded_like  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402
from imagestitch_amd import adjuster as adj  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_UNSUPPORTED, ERR_SIZE = 1, 2, 3, 6, 7
NAMED = cases.named()


def _case():
    c = cases.join([dict(NAMED["camera_without_edge"], max_iter=3), NAMED["max_iter_3"]])      # 7 images, 9 pairs, rig_first [0, 4, 7]
    c["refine_flags"] = 29
    return c


def _call(c, ins, outs, stream=None, **over):
    n, npairs = len(c["sizes"]), len(c["pairs"])
    a = dict(img_sizes=c["sizes"], keypoints=[ins["kp%d" % i].view for i in range(n)], pairs=c["pairs"], matches=[ins["mt%d" % p].view for p in range(npairs)],
             masks=[ins["mk%d" % p].view for p in range(npairs)], counts=ins["counts"].view, stats=ins["stats"].view, conf=ins["conf"].view,
             est_rig_stats=ins["est"].view, cameras_in=ins["cin"].view, cameras_out=outs["cameras_out"].view, kr32_out=outs["kr32_out"].view,
             rig_stats_out=outs["rig_stats_out"].view, rig_err_out=outs["rig_err_out"].view, rig_first=c["rig_first"], conf_thresh=c["conf_thresh"],
             max_iter=c["max_iter"], refine_flags=c["refine_flags"], stream=stream)
    a.update(over)
    return adj.bundle_adjust_reproj(**a)


@pytest.mark.parametrize("where,layout", [("device", "aligned"), ("device", "odd"), ("host", "odd"), ("host", "aligned")])
def test_a_call_writes_its_outputs_and_nothing_beside_them(gpu, where, layout):
    import torch
    c = _case()
    ins, outs = ray._mats(c, where, layout)
    assert _call(c, ins, outs) == (2, 1)
    torch.cuda.synchronize()
    for g in ins.values():
        g.check(written=NOTHING)
    for g in outs.values():
        g.check()
    want = fz.run_model(c)
    for g, w in zip(outs.values(), want):
        assert fz.same(g.get(), w) and not np.isnan(w.astype(np.float64)).any(), g.name


@pytest.mark.parametrize("where", ["device", "host"])
def test_refusals_write_not_one_byte(gpu, where):
    c = _case()
    ins, outs = ray._mats(c, where, "aligned", 20)
    n = len(c["sizes"])
    own = [("refine_flags -1", ERR_INVALID, dict(refine_flags=-1)), ("refine_flags 32", ERR_INVALID, dict(refine_flags=32))]
    for name, code, over in ray._refusals(c) + own:
        big = outs
        if "65 images" in name:      # outputs large enough, so that the rig's size alone is what is refused
            big = dict(cameras_out=guarded((67, 16), np.float64, where, "aligned", 31), kr32_out=guarded((67, 18), np.float32, where, "aligned", 32),
                       rig_stats_out=guarded((2, 8), np.int32, where, "aligned", 33), rig_err_out=guarded((2, 2), np.float64, where, "aligned", 34))
        with pytest.raises(_lib.IsxError) as e:
            _call(c, ins, big, **over)
        assert e.value.code == code, (name, e.value)
        ray._untouched(ins, big)
    with pytest.raises(_lib.IsxError) as e:                        # the Python wrapper's own: not an integer, before any device call
        _call(c, ins, outs, refine_flags=3.0)
    assert e.value.code == ERR_INVALID
    for key, shape, dtype, code in (("cameras_out", (n, 15), np.float64, ERR_SIZE), ("kr32_out", (n - 1, 18), np.float32, ERR_SIZE),
                                    ("rig_stats_out", (1, 8), np.int32, ERR_SIZE), ("rig_err_out", (2, 2), np.float32, ERR_TYPE),
                                    ("rig_err_out", (2, 1), np.float64, ERR_SIZE), ("kr32_out", (n, 18), np.int32, ERR_TYPE)):
        g = guarded(shape, dtype, where, "aligned", 40, key)
        with pytest.raises(_lib.IsxError) as e:
            _call(c, ins, outs, **{key: g.view})
        assert e.value.code == code, (key, shape, e.value)
        ray._untouched(ins, outs)
        g.check(written=NOTHING)


def test_null_pointers_are_refused(gpu):
    c = _case()
    ins, outs = ray._mats(c, "device", "aligned", 50)
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
            C.c_double(2.0 ** -52), 31, one["cameras_out"], one["kr32_out"], one["rig_stats_out"], one["rig_err_out"], None, 0, C.c_void_p(0)]
    for at in (1, 2, 4, 5, 6, 7, 8, 9, 12, 13, 18, 19, 20, 21):
        args = list(full)
        args[at] = None
        assert lib.isx_bundle_adjust_reproj(*args) == ERR_INVALID, at
        ray._untouched(ins, outs)
    args = list(full)
    args[11] = None                      # two rigs without rig_first
    assert lib.isx_bundle_adjust_reproj(*args) == ERR_INVALID
    ray._untouched(ins, outs)
    assert lib.isx_bundle_adjust_reproj(*full) == 0


def _capture_refused(call):
    """`call(stream)` raises ISX_ERR_STATE inside a capture on `stream`, and the capture stays intact."""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        x.add_(1.0)
        with pytest.raises(_lib.IsxError) as e:
            call(s)
        assert e.value.code == ERR_STATE and "captur" in e.value.msg
    torch.cuda.synchronize()
    assert float(x[0]) == 0.0                                      # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    return s


def test_a_capturing_stream_is_refused_with_nothing_enqueued(gpu):
    c = _case()
    ins, outs = ray._mats(c, "device", "aligned", 60)
    s = _capture_refused(lambda st: _call(c, ins, outs, stream=st))
    ray._untouched(ins, outs)
    assert _call(c, ins, outs, stream=s) == (2, 1)                 # the same stream works after the capture
    s.synchronize()
    want = fz.run_model(c)
    assert all(fz.same(g_.get(), w) for g_, w in zip(outs.values(), want))
    adj.release()


# ---- isx_wave_correct ------------------------------------------------------------------------------------------------------------------------
def _wave_case():
    rigs = cases.wave_rigs()
    names = ["pan_3", "one_image", "flip", "degenerate"]
    cams = np.concatenate([rigs[k] for k in names])
    return cams, [0] + [int(v) for v in np.cumsum([rigs[k].shape[0] for k in names])]


def _wave_mats(cams, nrigs, where, layout, seed):
    n = cams.shape[0]
    return (guarded_like(cams, where, layout, seed, "cameras_in"),
            dict(cameras_out=guarded((n, 16), np.float64, where, layout, seed + 1, "cameras_out"), kr32_out=guarded((n, 18), np.float32, where, layout, seed + 2, "kr32_out"),
                 rig_stats_out=guarded((nrigs, 2), np.int32, where, layout, seed + 3, "rig_stats_out")))


def _wave_call(cin, outs, first, kind=0, stream=None, **over):
    a = dict(cameras_in=cin.view, cameras_out=outs["cameras_out"].view, kr32_out=outs["kr32_out"].view, rig_stats_out=outs["rig_stats_out"].view,
             rig_first=first, kind=kind, stream=stream)
    a.update(over)
    return adj.wave_correct(**a)


@pytest.mark.parametrize("where,layout", [("device", "aligned"), ("device", "odd"), ("host", "odd"), ("host", "aligned")])
def test_wave_correct_writes_its_outputs_and_nothing_beside_them(gpu, where, layout):
    import torch
    cams, first = _wave_case()
    cin, outs = _wave_mats(cams, len(first) - 1, where, layout, 70)
    assert _wave_call(cin, outs, first, 1) == (4, 1)
    torch.cuda.synchronize()
    cin.check(written=NOTHING)
    for g in outs.values():
        g.check()
    for g, w in zip(outs.values(), rp.wave_correct(cams, first, 1)):
        assert fz.same(g.get(), w), g.name


@pytest.mark.parametrize("where", ["device", "host"])
def test_wave_correct_refusals_write_not_one_byte(gpu, where):
    cams, first = _wave_case()
    n, nrigs = cams.shape[0], len(first) - 1
    cin, outs = _wave_mats(cams, nrigs, where, "aligned", 80)
    raw = np.zeros(n * 16 * 8 + 16, np.uint8)
    refusals = [
        ("kind 2", ERR_INVALID, dict(kind=2)),
        ("kind -1", ERR_INVALID, dict(kind=-1)),
        ("rig_first not increasing", ERR_INVALID, dict(rig_first=[0, 3, 3, n])),
        ("rig_first past the images", ERR_INVALID, dict(rig_first=[0, 3, n + 1])),
        ("rig_first not from 0", ERR_INVALID, dict(rig_first=[1, 3, n])),
        ("no image", ERR_INVALID, dict(cameras_in=np.zeros((0, 16)), rig_first=None)),
        ("a misaligned cameras_in", ERR_INVALID, dict(cameras_in=np.frombuffer(raw, np.float64, n * 16, 4).reshape(n, 16))),
        ("cameras_in of another type", ERR_TYPE, dict(cameras_in=cams.astype(np.float32))),
        ("cameras_in with 15 columns", ERR_SIZE, dict(cameras_in=np.zeros((n, 15)))),
        ("cameras_out too short", ERR_SIZE, dict(cameras_out=np.zeros((n - 1, 16)))),
        ("kr32_out of another type", ERR_TYPE, dict(kr32_out=np.zeros((n, 18)))),
        ("kr32_out with 17 columns", ERR_SIZE, dict(kr32_out=np.zeros((n, 17), np.float32))),
        ("rig_stats_out with one column", ERR_SIZE, dict(rig_stats_out=np.zeros((nrigs, 1), np.int32))),
        ("rig_stats_out too short", ERR_SIZE, dict(rig_stats_out=np.zeros((nrigs - 1, 2), np.int32))),
    ]
    for name, code, over in refusals:
        with pytest.raises(_lib.IsxError) as e:
            _wave_call(cin, outs, first, **over)
        assert e.value.code == code, (name, e.value)
        ray._untouched({"cin": cin}, outs)
    lib = _lib.load()
    mats = [C.byref(_lib.as_mat(g.view)) for g in [cin] + list(outs.values())]
    f = (C.c_int * len(first))(*first)
    full = [n, nrigs, f, mats[0], 0, mats[1], mats[2], mats[3], None, 0, C.c_void_p(0)]
    for at in (2, 3, 5, 6, 7):                                     # several rigs without rig_first; null mats
        args = list(full)
        args[at] = None
        assert lib.isx_wave_correct(*args) == ERR_INVALID, at
        ray._untouched({"cin": cin}, outs)
    assert lib.isx_wave_correct(*full) == 0


def test_wave_correct_on_a_capturing_stream_is_refused(gpu):
    cams, first = _wave_case()
    cin, outs = _wave_mats(cams, len(first) - 1, "device", "aligned", 90)
    s = _capture_refused(lambda st: _wave_call(cin, outs, first, stream=st))
    ray._untouched({"cin": cin}, outs)
    assert _wave_call(cin, outs, first, stream=s) == (4, 1)
    s.synchronize()
    for g, w in zip(outs.values(), rp.wave_correct(cams, first, 0)):
        assert fz.same(g.get(), w), g.name
    adj.release()
