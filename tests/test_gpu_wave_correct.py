"""isx_wave_correct (imagestitch_amd/adjuster.py) on the GPU against wave_correct of tests/helpers/bundle_reproj_np.py by bits: rigs of 1,
2, 3, 5 and 64 images, both kinds, the conf < 0 flip and the degenerate rig; all of them as the rigs of one launch; host, device and strided
mats; cameras_out on top of cameras_in."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_reproj_cases as cases  # noqa: E402
from fuzz_estimator import place, same  # noqa: E402
from helpers import bundle_reproj_np as rp  # noqa: E402

pytestmark = pytest.mark.gpu
RIGS = cases.wave_rigs()
KINDS = (rp.WAVE_HORIZ, rp.WAVE_VERT)


def run_library(cams_in, rig_first, kind, layout="device"):
    import torch
    from imagestitch_amd import adjuster as adj
    n = cams_in.shape[0]
    nrigs = 1 if rig_first is None else len(rig_first) - 1
    outs = [place(np.zeros((n, 16)), layout, -7777.25), place(np.zeros((n, 18), np.float32), layout, -7777.25), place(np.zeros((nrigs, 2), np.int32), layout, -7777)]
    info = adj.wave_correct(place(cams_in, layout), *outs, rig_first=rig_first, kind=kind)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() if hasattr(o, "cpu") else o for o in outs), info


def check(got, want, what):
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and same(g, w), (what, g, w)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(RIGS))
def test_named_rigs(gpu, name, kind):
    cams = RIGS[name]
    got, info = run_library(cams, None, kind)
    want = rp.wave_correct(cams, None, kind)
    check(got, want, (name, kind))
    assert info == (1, 1) and got[2][0, 1] == cams.shape[0]
    assert same(got[0][:, 0:4], cams[:, 0:4]) and same(got[0][:, 13:16], cams[:, 13:16])      # focal, aspect, ppx, ppy and t are copied
    status = {"one_image": rp.WAVE_SINGLE, "degenerate": rp.WAVE_DEGENERATE}.get(name, 0)
    assert got[2][0, 0] == status
    assert same(got[0], cams) == (status != 0)                 # a rig passes through exactly where its status says so
    if name == "flip":
        assert rp.wave_matrix([c[4:13] for c in cams], rp.WAVE_HORIZ)[2] and not rp.wave_matrix([c[4:13] for c in cams], rp.WAVE_VERT)[2]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", ["host", "device", "strided"])
def test_every_rig_in_one_launch_in_every_layout(gpu, layout, kind):
    names = sorted(RIGS)
    cams = np.concatenate([RIGS[k] for k in names])
    first = [0] + [int(v) for v in np.cumsum([RIGS[k].shape[0] for k in names])]
    got, info = run_library(cams, first, kind, layout)
    assert info == (len(names), 1)
    check(got, rp.wave_correct(cams, first, kind), (layout, kind))
    at = 0
    for k, name in enumerate(names):                           # and each rig equals the rig alone
        alone = rp.wave_correct(RIGS[name], None, kind)
        m = RIGS[name].shape[0]
        assert same(got[0][at:at + m], alone[0]) and same(got[1][at:at + m], alone[1]) and np.array_equal(got[2][k], alone[2][0]), name
        at += m


def test_cameras_out_may_be_cameras_in(gpu):
    import torch
    from imagestitch_amd import adjuster as adj
    cams = RIGS["pan_64"]
    t = torch.from_numpy(cams.copy()).cuda()
    kr, rs = torch.zeros((64, 18), dtype=torch.float32, device="cuda"), torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    assert adj.wave_correct(t, t, kr, rs) == (1, 1)
    torch.cuda.synchronize()
    check((t.cpu().numpy(), kr.cpu().numpy(), rs.cpu().numpy()), rp.wave_correct(cams), "in place")
    adj.release()
