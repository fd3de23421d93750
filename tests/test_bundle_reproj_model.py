"""tests/helpers/bundle_reproj_np.py, the specification of isx_bundle_adjust_reproj and isx_wave_correct, on known answers - no GPU: the
compact Jacobian against the dense one; a cleared refinement bit; planted rigs of 2, 3 and 5 cameras run to their natural end, where the same
loop solved by np.linalg.lstsq guards the Cholesky decision; wave_correct against a float64 restatement with np.linalg.eigh, its matrix, a
planted pan about a tilted axis, both kinds, the conf < 0 flip, the degenerate rig and a rig of one image; the two entries in the header, in
_SIGS and in the Python wrappers' argument checks; the fuzz generator."""
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_math_cases as mc  # noqa: E402
import bundle_reproj_cases as cases  # noqa: E402
import fuzz_bundle_reproj as fz  # noqa: E402
from helpers import bundle_reproj_np as rp  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402
from imagestitch_amd import adjuster as adj  # noqa: E402

NAMED = cases.named()
WAVE = cases.wave_rigs()
WAVE_RUN = [k for k in sorted(WAVE) if k not in ("one_image", "degenerate")]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rig_and_param(c, flags=None):
    n = len(c["sizes"])
    edges = rp.gather_edges(c["keypoints"], c["pairs"], c["matches"], c["masks"], c["counts"].ravel(), c["conf"].ravel(), c["conf_thresh"])
    param = []
    for i in range(n):
        Q, _ = rp.polar([rp._f32(v) for v in c["cameras_in"][i, 4:13]])
        ci = c["cameras_in"][i]
        param += [float(ci[0]), float(ci[2]), float(ci[3]), float(ci[1])] + [rp._f32(v) for v in rp.rodrigues_vec(Q)]
    return rp.Rig(n, edges, c["refine_flags"] if flags is None else flags), param


# ---- the Jacobian ---------------------------------------------------------------------------------------------------------------------------
def _one_edge_a_camera():
    """Four cameras, the edges (0, 1) and (2, 3): (1, 2) lies below the threshold."""
    return cases.make(4, [(0, 1), (1, 2), (2, 3)], 20, inliers=[9, 5, 12], conf=[2.0, 0.5, 2.0])


@pytest.mark.parametrize("flags", [31, 21, 0])
def test_the_compact_jacobian_gives_the_bits_of_the_dense_one(flags):
    """J whole (2 matches x 7n, zeros multiplied) against the compact rows and their tiles.  Where every camera has one edge of one tile the
    two are the same running sums: J^T J and J^T err agree bit for bit.  Where a camera has several edges the model adds per-edge sums -
    another order, the same value to rounding - and the blocks of one edge alone still agree by bits."""
    for c in (NAMED["two_images_8_inliers"], _one_edge_a_camera()):
        rig, p = _rig_and_param(c, flags)
        assert all(len(e[2]) <= rp.TILE for e in rig.edges) and len(rig.edges) * 2 == rig.n
        JtJ, JtErr, enorm = rig.jac_err(p)
        dJtJ, dJtErr = rig.dense_jtj(p)
        assert np.array_equal(_bits(JtJ), _bits(dJtJ)) and np.array_equal(_bits(JtErr), _bits(dJtErr))
        assert enorm == rig.err_norm(p) and enorm > 0          # calcError after calcJacobian: the same bits
        J = np.array(JtJ)
        assert np.array_equal(J, J.T) and J.shape == (7 * rig.n, 7 * rig.n)
        for cam in range(rig.n):                               # the columns of a cleared bit are zero, the others are not
            for q in range(7):
                assert (J[7 * cam + q, 7 * cam + q] > 0) == rp.refined(flags, q), (cam, q)
        if rig.n == 4:
            assert not J[0:14, 14:28].any() and J[0:7, 7:14].any() and J[14:21, 21:28].any()
    rig, p = _rig_and_param(NAMED["max_iter_1"], flags)        # three cameras, all pairs
    J, g, _ = rig.jac_err(p)
    dJ, dg = rig.dense_jtj(p)
    assert np.allclose(J, dJ, rtol=1e-12, atol=0) and np.allclose(g, dg, rtol=1e-9, atol=1e-6)
    assert np.array_equal(_bits(np.array(J)[0:7, 7:14]), _bits(np.array(dJ)[0:7, 7:14]))


def test_tiles_change_the_order_and_nothing_else():
    rig, p = _rig_and_param(cases.make(2, [(0, 1)], 22, inliers=2 * rp.TILE + 3, outliers=0.0))
    J, g, en = rig.jac_err(p)
    dJ, dg = rig.dense_jtj(p)
    assert not np.array_equal(_bits(J), _bits(dJ))
    assert np.allclose(J, dJ, rtol=1e-12, atol=0) and np.allclose(g, dg, rtol=1e-9, atol=1e-6) and en == rig.err_norm(p)


def test_a_tile_carries_120_sums():
    rig, p = _rig_and_param(NAMED["tiles_5"])
    tiles = rig.tile_sums(rig.jacobian(p))
    assert [len(t) for t in tiles] == [1, 1, 2, 3, 1, 2]
    assert all(len(blk) + len(g) + 1 == 120 and len(blk) == 105 for ts in tiles for (blk, g, s) in ts)


@pytest.mark.parametrize("flags,kept", [(rp.REFINE_ALL & ~rp.REFINE_FOCAL, 0), (rp.REFINE_ALL & ~rp.REFINE_PPX, 2), (rp.REFINE_ALL & ~rp.REFINE_PPY, 3),
                                        (rp.REFINE_ALL & ~rp.REFINE_ASPECT, 1)])
def test_a_cleared_refinement_bit_keeps_its_parameter_and_sets_dropped(flags, kept):
    c = dict(NAMED["max_iter_3"], refine_flags=flags)
    cams, kr, rs, re = fz.run_model(c)
    assert rs[0, rp.RIG_STATUS] == rp.ST_DROPPED and rs[0, rp.RIG_ITERS] == 3
    assert np.array_equal(_bits(cams[:, kept]), _bits(c["cameras_in"][:, kept]))                  # column `kept` of cameras: untouched
    others = [k for k in range(4) if k != kept]
    assert not (cams[:, others] == c["cameras_in"][:, others]).any() and re[0, 1] < re[0, 0]
    full = fz.run_model(dict(c, refine_flags=rp.REFINE_ALL))
    assert full[2][0, rp.RIG_STATUS] == 0 and not (full[0][:, kept] == c["cameras_in"][:, kept]).any()
    unused = fz.run_model(dict(c, refine_flags=flags | 2))                                         # bit 1, (0,1), is not read
    assert all(fz.same(a, b) for a, b in zip(unused, (cams, kr, rs, re)))


# ---- planted rigs: the Cholesky solve against the lstsq one ---------------------------------------------------------------------------------
PLANTED = {2: ([(0, 1)], 30), 3: (cases.all_pairs(3), 20), 5: (cases.all_pairs(5), 12)}      # the rigs of tests/test_bundle_model.py, offsets planted


def _planted(n):
    pairs, inl = PLANTED[n]
    return cases.make(n, pairs, 100 + n, inliers=inl, outliers=0.2, off_deg=1.0, off_focal=0.05, max_iter=1000, r_scale=1.0)


def _distance(out, c):
    """How far a run's cameras lie from the planted ones: the largest relative focal error and the largest rotation angle (degrees)."""
    focal, Rs = c["planted"][0], c["planted"][1]
    cams = out["cameras"]
    df = max(abs(cams[i, 0] - focal) / focal for i in range(len(Rs)))
    ang = 0.0
    for i, R in enumerate(Rs):
        D = cams[i, 4:13].reshape(3, 3) @ np.asarray(R).T
        ang = max(ang, float(np.degrees(np.arccos(np.clip((np.trace(D) - 1) / 2, -1, 1)))))
    return df, ang


@functools.lru_cache(maxsize=None)
def _runs(n):
    c = _planted(n)
    a = (c["sizes"], c["keypoints"], c["pairs"], c["matches"], c["masks"], c["counts"].ravel(), c["conf"].ravel(), c["est_rig_stats"][0], c["cameras_in"],
         c["conf_thresh"], c["max_iter"], rp.DBL_EPSILON, c["refine_flags"])
    return c, rp.adjust_rig(*a, solve=rp.chol_solve), rp.adjust_rig(*a, solve=rp.lstsq_solve)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_planted_rigs_end_where_the_lstsq_solve_ends(n):
    """Known focal (900), principal point, aspect 1 and rotations; exact projections rounded to float32 keypoints; cameras started 1 degree
    and 5 % off with ppx, ppy moved by 6 and 4 pixels and the aspect scaled by 1 %.  THE GUARD ON THE CHOLESKY DECISION: the same loop with
    np.linalg.lstsq as its solve is the reference; the Cholesky run's last |err| is at most 1 % above its.  No recovery tolerance is fixed in
    advance - two or three cameras do not pin focal, principal point and aspect, and both solves end equally far from the planted values: the
    lstsq run's distance is measured and the Cholesky run must lie within twice it.  Measured here (first |err|; last |err| Cholesky, lstsq;
    iterations; the distance from the planted cameras as (largest relative focal error, largest rotation angle in degrees)):
       n = 2: 271.079; 1.5419502232e-4, 1.5419502234e-4; 11, 6; Cholesky (7.5970e-3, 0.10889), lstsq (7.5970e-3, 0.10889)
       n = 3: 424.551; 3.0707065882e-4, 3.0707065876e-4; 7, 8;  Cholesky (1.0654e-2, 0.43752), lstsq (1.0654e-2, 0.43752)
       n = 5: 626.850; 3.3507784607e-4, 3.3507784597e-4; 9, 12; Cholesky (6.2546e-7, 0.005852), lstsq (6.2546e-7, 0.012862)"""
    c, chol, lsq = _runs(n)
    first, last_c, last_l = chol["rig_err"][0], chol["rig_err"][1], lsq["rig_err"][1]
    dc, dl = _distance(chol, c), _distance(lsq, c)
    print("n", n, "first", first, "last chol", last_c, "last lstsq", last_l, "distance chol", dc, "lstsq", dl, "iters", chol["info"]["iters"], lsq["info"]["iters"])
    assert chol["rig_stats"][rp.RIG_STATUS] & ~rp.ST_DROPPED == 0 and chol["info"]["iters"] < 1000
    assert last_c <= 1.01 * last_l, (last_c, last_l)
    assert last_c < first / 1e4
    for k in range(2):
        assert dc[k] <= 2.0 * dl[k], (k, dc, dl)


# ---- wave_correct ---------------------------------------------------------------------------------------------------------------------------
def _wave64(cams, kind):
    """waveCorrect in float64 with np.linalg.eigh (on the float32-rounded R, as the input of the float32 path is)."""
    Rs = [np.asarray(c[4:13], np.float32).astype(np.float64).reshape(3, 3) for c in cams]
    moment = sum(np.outer(R[:, 0], R[:, 0]) for R in Rs)
    w, v = np.linalg.eigh(moment)                              # ascending, eigenvectors as columns
    rg1 = v[:, 0] if kind == rp.WAVE_HORIZ else v[:, 2]
    k = sum(R[:, 2] for R in Rs)
    rg0 = np.cross(rg1, k)
    rg0 /= np.linalg.norm(rg0)
    rg2 = np.cross(rg0, rg1)
    conf = sum(rg0 @ R[:, 0] for R in Rs) if kind == rp.WAVE_HORIZ else -sum(rg1 @ R[:, 0] for R in Rs)
    if conf < 0:
        rg0, rg1 = -rg0, -rg1
    Rw = np.stack([rg0, rg1, rg2])
    return Rw, [Rw @ R for R in Rs]


def _wave_deviation():
    """The largest deviation of an output R entry of the float32 path from the float64 restatement over the named rigs, both kinds."""
    worst = {}
    for name in WAVE_RUN:
        for kind in (rp.WAVE_HORIZ, rp.WAVE_VERT):
            got = rp.wave_correct(WAVE[name], None, kind)[0]
            _, want = _wave64(WAVE[name], kind)
            worst[(name, kind)] = max(np.abs(got[i, 4:13].reshape(3, 3) - want[i]).max() for i in range(len(want)))
    return worst


# measured over the named rigs, both kinds: 1.8e-7 at the most on nine of the ten - a dozen float32 roundings on entries of magnitude 1 - and
# 1.991e-5 on pan_64 with VERT, a correction that means little on a horizontal sweep: there rg1 lies 0.44 degrees from the sum of the z axes, so
# rg0 = rg1 x img_k has a norm of 0.06 beside factors of norm 1 and 7.8 and dividing by it multiplies their float32 rounding by 130; the tests
# below allow four times the largest
WAVE_DEVIATION = 1.991e-5
WAVE_BOUND = 4.0 * WAVE_DEVIATION


def test_wave_correct_against_the_float64_restatement():
    worst = _wave_deviation()
    print("largest deviation of an R entry:", worst)
    assert 0 < max(worst.values()) <= WAVE_BOUND


@pytest.mark.parametrize("kind", [rp.WAVE_HORIZ, rp.WAVE_VERT])
@pytest.mark.parametrize("name", WAVE_RUN)
def test_the_correction_is_a_rotation(name, kind):
    Rw, status, _ = rp.wave_matrix([c[4:13] for c in WAVE[name]], kind)
    M = np.array(Rw, np.float64).reshape(3, 3)
    assert status == 0 and all(isinstance(v, np.float32) for v in Rw)
    assert np.abs(M @ M.T - np.eye(3)).max() <= WAVE_BOUND and abs(np.linalg.det(M) - 1.0) <= WAVE_BOUND


def test_a_pan_about_a_tilted_axis_comes_out_level():
    cams = WAVE["pan_5_planted"]
    before = max(abs(c[4:13].reshape(3, 3)[1, 0]) for c in cams)
    out = rp.wave_correct(cams, None, rp.WAVE_HORIZ)[0]
    after = max(abs(c[4:13].reshape(3, 3)[1, 0]) for c in out)
    print("largest |y| of a column 0: before", before, "after", after)
    assert before > 0.05 and after <= WAVE_BOUND              # every camera's x axis lies in the horizontal plane
    assert min(c[4:13].reshape(3, 3)[0, 0] for c in out) > 0  # and points the way it did


def test_vert_and_horiz_differ_and_everything_but_R_is_copied():
    cams = WAVE["pan_5_planted"]
    h, v = rp.wave_correct(cams, None, rp.WAVE_HORIZ), rp.wave_correct(cams, None, rp.WAVE_VERT)
    assert np.abs(h[0][:, 4:13] - v[0][:, 4:13]).max() > 0.5
    for out in (h, v):
        assert np.array_equal(_bits(out[0][:, 0:4]), _bits(cams[:, 0:4])) and np.array_equal(_bits(out[0][:, 13:16]), _bits(cams[:, 13:16]))
        assert np.array_equal(out[1][:, 9:18], out[0][:, 4:13].astype(np.float32)) and out[2].tolist() == [[0, 5]]
        assert np.array_equal(out[1][:, 0], cams[:, 0].astype(np.float32)) and np.array_equal(out[1][:, 4], (cams[:, 0] * cams[:, 1]).astype(np.float32))


def test_the_flip_the_degenerate_rig_and_one_image():
    flip = [c[4:13] for c in WAVE["flip"]]
    Rw, status, flipped = rp.wave_matrix(flip, rp.WAVE_HORIZ)
    assert status == 0 and flipped and not rp.wave_matrix([c[4:13] for c in WAVE["pan_5_planted"]], rp.WAVE_HORIZ)[2]
    out = rp.wave_correct(WAVE["flip"], None, rp.WAVE_HORIZ)[0]
    assert min(c[4:13].reshape(3, 3)[0, 0] for c in out) > 0                                       # the x axes point along +x after the flip
    for name, bit in (("degenerate", rp.WAVE_DEGENERATE), ("one_image", rp.WAVE_SINGLE)):
        for kind in (rp.WAVE_HORIZ, rp.WAVE_VERT):
            cams, kr, rs = rp.wave_correct(WAVE[name], None, kind)
            assert rs.tolist() == [[bit, WAVE[name].shape[0]]] and np.array_equal(_bits(cams), _bits(WAVE[name]))
            assert np.array_equal(kr[:, 9:18], WAVE[name][:, 4:13].astype(np.float32))
    both = np.concatenate([WAVE["one_image"], WAVE["pan_3"], WAVE["degenerate"]])                 # rigs of one call are independent
    cams, kr, rs = rp.wave_correct(both, [0, 1, 4, 6], rp.WAVE_HORIZ)
    assert rs.tolist() == [[rp.WAVE_SINGLE, 1], [0, 3], [rp.WAVE_DEGENERATE, 2]]
    assert np.array_equal(_bits(cams[1:4]), _bits(rp.wave_correct(WAVE["pan_3"], None, rp.WAVE_HORIZ)[0]))


def test_the_float32_jacobi_gives_eigenpairs():
    rng = np.random.default_rng(3)
    for _ in range(20):
        B = rng.normal(size=(3, 3)).astype(np.float32)
        A = (B @ B.T).astype(np.float32)
        W, V = rp.jacobi3_f32(A)
        W, V = np.array(W, np.float64), np.array(V, np.float64)
        assert all(isinstance(w, np.float32) for w in rp.jacobi3_f32(A)[0]) and W[0] >= W[1] >= W[2]
        assert np.abs(V @ A.astype(np.float64) - W[:, None] * V).max() <= 2e-5 * max(1.0, W[0])


# ---- the rigs that go round ---------------------------------------------------------------------------------------------------------------------
def test_which_branches_the_named_cases_take():
    """tests/test_bundle_model.py's condition under this adjuster: every rig of bundle_cases.WIDE takes, in the model, the branches of
    bundle_math.hpp it was written for (so tests/test_gpu_bundle_reproj.py runs them on the device), and no narrow named case takes
    |x| < 0.5 or x <= -0.5 of acos, the half turn of cvRodrigues2 or det < 0 of the polar factor."""
    assert set(cases.WIDE) == set(mc.WIDE_TAKES) <= set(NAMED)
    for name, c in NAMED.items():
        with mc.BranchCounter() as b:
            fz.run_model(c)
        if name in mc.WIDE_TAKES:
            assert all(b.taken[k] >= 1 for k in mc.WIDE_TAKES[name]), (name, b.taken)
        else:
            assert all(b.taken[k] == 0 for k in mc.NARROW_NEVER), (name, b.taken)
    assert rp.polar is rp.bm.polar and rp.rodrigues_vec is rp.bm.rodrigues_vec and rp.polar.__module__ == rp.bm.__name__      # the counters are gone


# ---- the entries ----------------------------------------------------------------------------------------------------------------------------
def _declared(name):
    text = open(os.path.join(ROOT, "include", "imagestitch_hip.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [a.strip() for a in args.split(",")]


def test_both_entries_are_declared_and_in_sigs_with_matching_arity():
    ray, reproj, wave = _declared("isx_bundle_adjust_ray"), _declared("isx_bundle_adjust_reproj"), _declared("isx_wave_correct")
    assert len(reproj) == len(_lib._SIGS["isx_bundle_adjust_reproj"]) == len(ray) + 1 == len(_lib._SIGS["isx_bundle_adjust_ray"]) + 1
    at = reproj.index("int refine_flags")
    assert reproj[at + 1] == "isx_mat* cameras_out" and reproj[:at] + reproj[at + 1:] == ray
    assert _lib._SIGS["isx_bundle_adjust_reproj"][at] is _lib.C.c_int
    assert len(wave) == len(_lib._SIGS["isx_wave_correct"]) == 11
    assert {"isx_bundle_adjust_reproj", "isx_wave_correct"} <= set(_lib.declared_symbols())
    host, dev = _declared("isx_selftest_bundle_math"), _declared("isx_selftest_bundle_math_device")      # the self-test and its device twin
    assert host == dev and len(dev) == len(_lib._SIGS["isx_selftest_bundle_math_device"]) == 4
    assert _lib._SIGS["isx_selftest_bundle_math_device"] == _lib._SIGS["isx_selftest_bundle_math"]
    assert "isx_selftest_bundle_math_device" in _lib.declared_symbols()
    import imagestitch_amd as I
    for name in ("BundleAdjusterReproj", "bundle_adjust_reproj", "wave_correct", "waveCorrect", "WAVE_CORRECT_HORIZ", "WAVE_CORRECT_VERT"):
        assert hasattr(I, name) and name in I.__all__, name
    assert (I.WAVE_CORRECT_HORIZ, I.WAVE_CORRECT_VERT) == (0, 1) and issubclass(I.BundleAdjusterReproj, adj._BundleAdjusterBase)
    assert issubclass(I.BundleAdjusterRay, adj._BundleAdjusterBase)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", boom)
    z = np.zeros((2, 16))
    with pytest.raises(_lib.IsxError) as e:
        adj.bundle_adjust_reproj([(4, 4)] * 2, [z], [], [], [], z, z, z, z, z, z, z, z, z)          # one keypoints mat for two images
    assert e.value.code == 1
    with pytest.raises(_lib.IsxError) as e:
        adj.bundle_adjust_reproj([(4, 4)] * 2, [z, z], [], [], [], z, z, z, z, z, z, z, z, z, refine_flags=1.5)
    assert e.value.code == 1
    for bad in (np.ones((2, 3)), 32, -1, 2.0, "all"):
        with pytest.raises(_lib.IsxError) as e:
            adj.BundleAdjusterReproj().setRefinementMask(bad)
        assert e.value.code == 1
    ba = adj.BundleAdjusterReproj()
    assert ba.refine_flags == 31
    ba.setRefinementMask(np.array([[1, 0, 1], [0, 0, 1], [0, 0, 0]]))
    assert ba.refine_flags == rp.REFINE_FOCAL | rp.REFINE_PPX | rp.REFINE_PPY
    ba.setRefinementMask(9)
    assert ba.refine_flags == 9
    with pytest.raises(_lib.IsxError) as e:
        ba([(4, 4)] * 2, [z, z], object(), None)                                                   # a matcher that has not run
    assert e.value.code == 3 and "BundleAdjusterReproj" in e.value.msg
    with pytest.raises(_lib.IsxError) as e:
        adj.waveCorrect([], "diagonal")
    assert e.value.code == 1
    with pytest.raises(_lib.IsxError) as e:
        adj.waveCorrect(adj.BundleAdjusterReproj(), "horiz")                                       # an adjuster that has not run
    assert e.value.code == 3


# ---- the fuzz generator ---------------------------------------------------------------------------------------------------------------------
def test_the_fuzz_generator_is_deterministic_and_covers_its_classes():
    seen_flags, moved = set(), 0
    for s in range(24):
        a, b = fz.make_case(1000 + s), fz.make_case(1000 + s)
        assert a["refine_flags"] == b["refine_flags"] and np.array_equal(_bits(a["cameras_in"]), _bits(b["cameras_in"]))
        assert 0 <= a["refine_flags"] <= 31 and a["cls"] == fz.CLASSES[(1000 + s) % len(fz.CLASSES)] and a["max_iter"] <= 40
        seen_flags.add(a["refine_flags"])
        moved += bool((a["cameras_in"][:, 1] != 1.0).any())
    assert {0, 31} <= seen_flags and len(seen_flags) >= 5 and 0 < moved < 24
    c = fz.make_case(1003)
    assert all(fz.same(x, y) for x, y in zip(fz.run_model(c), fz.run_model(fz.make_case(1003))))
