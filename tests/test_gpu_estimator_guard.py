"""isx_estimate_cameras writes its outputs and nothing beside them, and a refused call writes nothing at all: every mat lies inside the
guard bands of tests/helpers/guarded.py.  Each refusal of the header - null pointers, one image in a rig, from >= to, a repeated pair, a
pair across two rigs, an index out of range, rig_first not increasing, a misaligned mat, another type, too few rows or columns, more than
64 images in a rig, a capturing stream - with host and device outputs."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import estimator_cases as cases  # noqa: E402
import fuzz_estimator as fz  # noqa: E402
from helpers import estimator_np as em  # noqa: E402
from helpers.guarded import NOTHING, guarded, guarded_like  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402
from imagestitch_amd import cameras as cam  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_TYPE, ERR_STATE, ERR_UNSUPPORTED, ERR_SIZE = 1, 2, 3, 6, 7
NAMED = cases.named()


def _case():
    return cases.join([NAMED["complete_5"], NAMED["chain_3"]])          # 8 images, 12 pairs, rig_first [0, 5, 8]


def _mats(c, where, layout, seed=1):
    """Inputs (holding the case) and outputs (random bytes) inside guard bands."""
    n, npairs, nrigs = len(c["sizes"]), len(c["pairs"]), len(c["rig_first"]) - 1
    ins = dict(H=guarded_like(np.asarray(c["H"], np.float64).reshape(3 * npairs, 3), where, layout, seed, "H"),
               stats=guarded_like(c["stats"], where, layout, seed + 1, "stats"),
               conf=guarded_like(np.zeros((1, npairs)), where, layout, seed + 2, "conf"))
    outs = dict(cameras=guarded((n, 16), np.float64, where, layout, seed + 3, "cameras"), kr32=guarded((n, 18), np.float32, where, layout, seed + 4, "kr32"),
                tree=guarded((n, 2), np.int32, where, layout, seed + 5, "tree"), rig_stats=guarded((nrigs, 8), np.int32, where, layout, seed + 6, "rig_stats"))
    return ins, outs


def _call(c, ins, outs, stream=None, **over):
    a = dict(img_sizes=c["sizes"], pairs=c["pairs"], H=ins["H"].view, stats=ins["stats"].view, conf=ins["conf"].view, cameras=outs["cameras"].view,
             kr32=outs["kr32"].view, tree=outs["tree"].view, rig_stats=outs["rig_stats"].view, rig_first=c["rig_first"], focals_in=None, stream=stream)
    a.update(over)
    return cam.estimate_cameras(**a)


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
    want = em.estimate(c["sizes"], c["pairs"], c["H"], c["stats"], c["rig_first"])
    for g, w in zip(outs.values(), want):
        assert fz.same(g.get(), w) and not np.isnan(w.astype(np.float64)).any(), g.name


def _refusals(c):
    """(name, status, overrides of _call's arguments)"""
    n, npairs = len(c["sizes"]), len(c["pairs"])
    p = list(c["pairs"])
    host_h = np.zeros(3 * npairs * 3 * 8 + 16, np.uint8)
    return [
        ("one image in a rig", ERR_INVALID, dict(rig_first=[0, 1, 8], pairs=[], )),
        ("from >= to", ERR_INVALID, dict(pairs=p[:3] + [(p[3][1], p[3][0])] + p[4:])),
        ("from == to", ERR_INVALID, dict(pairs=p[:3] + [(2, 2)] + p[4:])),
        ("a repeated pair", ERR_INVALID, dict(pairs=p[:-1] + [p[0]])),
        ("a pair across two rigs", ERR_INVALID, dict(pairs=p[:-1] + [(4, 5)])),
        ("an index out of range", ERR_INVALID, dict(pairs=p[:-1] + [(6, n)])),
        ("a negative index", ERR_INVALID, dict(pairs=p[:-1] + [(-1, 2)])),
        ("rig_first not increasing", ERR_INVALID, dict(rig_first=[0, 5, 3, 8], pairs=[])),
        ("rig_first past the images", ERR_INVALID, dict(rig_first=[0, 5, 9])),
        ("a misaligned H", ERR_INVALID, dict(H=np.frombuffer(host_h, np.float64, 3 * npairs * 3, 4).reshape(3 * npairs, 3))),
        ("stats of another type", ERR_TYPE, dict(stats=np.zeros((npairs, 8), np.float32))),
        ("H of another type", ERR_TYPE, dict(H=np.zeros((3 * npairs, 3), np.float32))),
        ("H with too few rows", ERR_SIZE, dict(H=np.zeros((3 * npairs - 1, 3)))),
        ("stats with one column", ERR_SIZE, dict(stats=np.zeros((npairs, 1), np.int32))),
        ("focals_in with three columns", ERR_SIZE, dict(focals_in=np.zeros((n, 3)))),
        ("65 images in a rig", ERR_UNSUPPORTED, dict(img_sizes=[(640, 480)] * 67, rig_first=[0, 65, 67], pairs=[])),
    ]


@pytest.mark.parametrize("where", ["device", "host"])
def test_refusals_write_not_one_byte(gpu, where):
    c = _case()
    ins, outs = _mats(c, where, "aligned", 20)
    n = len(c["sizes"])
    for name, code, over in _refusals(c):
        if "65 images" in name:      # outputs large enough, so that the rig's size alone is what is refused
            big = dict(cameras=guarded((67, 16), np.float64, where, "aligned", 31), kr32=guarded((67, 18), np.float32, where, "aligned", 32),
                       tree=guarded((67, 2), np.int32, where, "aligned", 33), rig_stats=guarded((2, 8), np.int32, where, "aligned", 34))
            with pytest.raises(_lib.IsxError) as e:
                _call(c, ins, big, **over)
            assert e.value.code == code, (name, e.value)
            _untouched(ins, big)
            continue
        with pytest.raises(_lib.IsxError) as e:
            _call(c, ins, outs, **over)
        assert e.value.code == code, (name, e.value)
        _untouched(ins, outs)
    # an output too small, of another type, misaligned: the other outputs stay untouched as well
    for key, shape, dtype, code in (("cameras", (n, 15), np.float64, ERR_SIZE), ("kr32", (n - 1, 18), np.float32, ERR_SIZE), ("tree", (n, 2), np.float32, ERR_TYPE),
                                    ("rig_stats", (1, 8), np.int32, ERR_SIZE), ("kr32", (n, 18), np.int32, ERR_TYPE)):
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
    mats = [C.byref(_lib.as_mat(g.view)) for g in list(ins.values()) + [None] + list(outs.values()) if g is not None]
    full = [n, sizes, npairs, pij, 2, first, mats[0], mats[1], mats[2], None, mats[3], mats[4], mats[5], mats[6], None, 0, C.c_void_p(0)]
    for at in (1, 3, 6, 7, 8, 10, 11, 12, 13):
        args = list(full)
        args[at] = None
        assert lib.isx_estimate_cameras(*args) == ERR_INVALID, at
        _untouched(ins, outs)
    args = list(full)
    args[5] = None                       # two rigs without rig_first
    assert lib.isx_estimate_cameras(*args) == ERR_INVALID
    _untouched(ins, outs)
    assert lib.isx_estimate_cameras(*full) == 0


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
    want = em.estimate(c["sizes"], c["pairs"], c["H"], c["stats"], c["rig_first"])
    assert all(fz.same(g_.get(), w) for g_, w in zip(outs.values(), want))
    cam.release()
