"""The NumPy specification of isx_find_homography_lm (tests/helpers/homography_lm_np.py) on its own: the n-general Jacobi against
homography_np.jacobi_scalar (bit for bit at 9) and np.linalg.eigh (at 8), solve and invert(DECOMP_EIG) against np.linalg, compute on a hand
case with a row whose ww is exactly 0, the grouped norm and dot by hand, that LM never raises S, that the named cases of
tests/homography_lm_cases.py together reach every branch of LMSolverImpl1::run and are not fragile, the header's arity, and that
tools/fuzz_homography.case() draws what it drew before --refine.  CPU only."""
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import homography_cases as cases  # noqa: E402
import homography_lm_cases as lmc  # noqa: E402
from helpers import homography_lm_np as lm  # noqa: E402
from helpers import homography_np as hm  # noqa: E402

NAMED = lmc.named()
_MODEL = {}


def model(name):
    if name not in _MODEL:
        pts, kw = NAMED[name]
        _MODEL[name] = lm.find_homography_lm_np(pts, **kw)
    return _MODEL[name]


def _ltl(name, rows=None):
    pts = cases.named()[name][0][:rows]
    ok, LtL, _, _ = hm.build_ltl(pts[None, :, 0:2], pts[None, :, 2:4])
    assert ok[0]
    return LtL[0]


def test_jacobi_n_is_jacobi_scalar_at_9_and_agrees_with_eigh_at_8():
    for name, rows in (("n6_exact", None), ("n65_half_noisy", None), ("n300_half_noisy", None), ("repeated_5x4", None), ("n65_half_noisy", 4)):
        A = _ltl(name, rows)
        W, V, rot = lm.jacobi_n(A, 9)
        Ws, Vs, rs = hm.jacobi_scalar(A)
        assert np.array_equal(np.array(W).view(np.uint64), np.array(Ws).view(np.uint64)) and rot == rs > 20
        assert np.array_equal(np.array(V).view(np.uint64), np.array(Vs).view(np.uint64))
        A8 = A[:8, :8]                                                # a principal minor: symmetric in its upper triangle as well
        full = np.triu(A8) + np.triu(A8, 1).T
        W8, V8, rot8 = lm.jacobi_n(A8, 8)
        w = np.linalg.eigvalsh(full)[::-1]
        assert 0 < rot8 < 8 * 8 * 30 and (np.diff(W8) <= 0).all()
        assert np.abs(np.array(W8) - w).max() <= 1e-9 * np.abs(w).max()            # the tolerance of the 9 x 9 test
        for e in range(8):
            v = np.array(V8[e])
            assert abs(np.linalg.norm(v) - 1) < 1e-12 and np.linalg.norm(full @ v - W8[e] * v) <= 1e-9 * np.linalg.norm(full)
    W, V, rot = lm.jacobi_n(np.diag(np.arange(8.0)), 8)               # nothing to rotate: sorted descending, V a permutation
    assert rot == 0 and W == list(np.arange(7.0, -1, -1)) and np.array_equal(np.array(V), np.eye(8)[::-1])


def _spd(seed):
    r = np.random.default_rng(seed)
    B = r.normal(size=(8, 8))
    return B @ B.T + 8.0 * np.eye(8), r.normal(size=8)               # well conditioned: eigenvalues in about [8, 40]


def test_solve_and_invert_eig_against_numpy():
    for seed in range(6):
        A, v = _spd(seed)
        assert np.linalg.cond(A) < 100
        rows = [list(map(float, row)) for row in A]
        d = np.array(lm.solve_eig(rows, [float(x) for x in v]))
        want = np.linalg.solve(A, v)
        assert np.abs(d - want).max() <= 1e-9 * np.abs(want).max()
        diag = np.array(lm.invert_eig_diag(rows))
        want = np.diag(np.linalg.inv(A))
        assert np.abs(diag - want).max() <= 1e-9 * np.abs(want).max()
    A = np.diag([4.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0])           # a zero eigenvalue is below the threshold: dropped, not divided by
    assert lm.solve_eig(A.tolist(), [4.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0, 5.0]) == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert lm.invert_eig_diag(A.tolist()) == [0.25, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0]


def test_compute_on_a_hand_case_and_the_zero_ww_branch():
    """h = a translation by (2, 3): ww = 1, (xi, yi) = (Mx + 2, My + 3).  Second row: h6 = -1 / Mx with Mx = 4, a power of two, so
    h6 Mx = -1 exactly and ww = (-1 + 0) + 1 = 0: R:436 takes the 0 branch, xi = yi = 0 and the row's Jacobian is zeros."""
    src, dst = np.array([[5, 7]], np.float32), np.array([[6.5, 11]], np.float32)
    err, J = lm.compute([1.0, 0.0, 2.0, 0.0, 1.0, 3.0, 0.0, 0.0], src, dst, True)
    assert err == [0.5, -1.0]
    assert J == [[5.0, 7.0, 1.0, 0.0, 0.0, 0.0, -35.0, -49.0], [0.0, 0.0, 0.0, 5.0, 7.0, 1.0, -50.0, -70.0]]
    err2, none = lm.compute([1.0, 0.0, 2.0, 0.0, 1.0, 3.0, 0.0, 0.0], src, dst, False)
    assert err2 == err and none is None
    h = [1.0, 0.0, 2.0, 0.0, 1.0, 3.0, -0.25, 0.0]
    src, dst = np.array([[5, 7], [4, 9]], np.float32), np.array([[6.5, 11], [1.5, -2.5]], np.float32)
    err, J = lm.compute(h, src, dst, True)
    assert err[2:] == [-1.5, 2.5] and all(v == 0.0 for row in J[2:] for v in row)
    ww = 1.0 / ((-0.25 * 5.0 + 0.0 * 7.0) + 1.0)                      # the first row is an ordinary one: ww = -4
    assert ww == -4.0 and err[:2] == [7.0 * ww - 6.5, 10.0 * ww - 11.0] and J[0][:3] == [-20.0, -28.0, -4.0] and J[0][6] == 20.0 * (7.0 * ww)
    A = lm.mul_transposed(J)                                          # the zero rows add +0.0 - or -0.0 to a sum that is not -0.0
    assert np.array_equal(np.array(A).view(np.uint64), np.array(lm.mul_transposed(J[:2])).view(np.uint64))


def test_the_sums_by_hand():
    big = 2.0 ** 53
    assert lm.norm_l2sqr([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]) == ((((1.0 + 4.0) + 9.0) + 16.0) + 25.0) + 36.0
    # the group of four is summed before it meets s
    v = [2.0 ** 27, 1.0, 1.0, 1.0, 2.0 ** 27, 1.0, 1.0, 1.0]
    g = ((2.0 ** 54 + 1.0) + 1.0) + 1.0                               # each + 1 is lost against 2^54
    assert g == 2.0 ** 54 and lm.norm_l2sqr(v) == (0.0 + g) + g == 2.0 ** 55
    assert lm.norm_l2sqr(v[:4] + [1.0, 1.0]) == (g + 1.0) + 1.0 and lm.norm_l2sqr([]) == 0.0
    assert lm.dot8([big, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0], [1.0] * 8) == (0.0 + ((big + 1.0) + 1.0)) + 2.0
    assert lm.norm_inf([1.0, -3.0, 2.0, float("nan")]) == 3.0 and lm.norm_inf([]) == 0.0
    J = [[1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 3.0, 4.0], [0.0, 0.0, 0.0, 5.0, 6.0, 1.0, 7.0, 8.0]]
    A = np.array(lm.mul_transposed(J))
    assert np.array_equal(A, np.array(J).T @ np.array(J)) and lm.gemm_1t(J, [2.0, -1.0]) == [2.0, 4.0, 0.0, -5.0, -6.0, -1.0, -1.0, 0.0]


def test_skipping_the_structural_zeros_gives_the_same_bits():
    for name in ("inliers_9", "noise25_invert", "translation_20"):
        pts = NAMED[name][0]
        H = hm.find_homography_np(pts, **{k: v for k, v in NAMED[name][1].items() if k != "lm_max_iters"})["H"].reshape(9)
        _, J = lm.compute(list(H[:8]), pts[:, 0:2], pts[:, 2:4], True)
        assert np.isfinite(np.array(J)).all()
        full, skipped = np.array(lm.mul_transposed(J)), np.array(lm.mul_transposed(J, skip_zeros=True))
        assert np.array_equal(full.view(np.uint64), skipped.view(np.uint64))


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases(name):
    """Not fragile; S never rises (exact); columns 0 - 7, the mask and conf are the unrefined model's unless DEGENERATE is flagged; H[8]
    keeps runKernel's bits where LM accepted nothing else of pass 2's refit."""
    pts, kw = NAMED[name]
    r = model(name)
    old = hm.find_homography_np(pts, **{k: v for k, v in kw.items() if k != "lm_max_iters"})
    assert r["margin"] >= 1e-9
    for S in r["S"]:
        if S is not None:
            assert S[1] <= S[0]
    if not (r["stats"][0] | old["stats"][0]) & lm.ST_DEGENERATE:
        assert np.array_equal(r["stats"][:8], old["stats"]) and r["conf"] == old["conf"]
        assert (r["mask"] is None and old["mask"] is None) or np.array_equal(r["mask"], old["mask"])
        assert r["H"][2, 2] == old["H"][2, 2]                        # H8 aliases eight doubles (R:669)
    ran = [c is not None for c in r["counters"]]
    assert ran == [bool(r["stats"][9]), bool(r["stats"][11])]
    if name in lmc.NO_LM:
        assert ran == [False, False] and r["stats"][8:].tolist() == [0, 0, 0, 0] and np.array_equal(r["H"], old["H"])
    else:
        assert ran[0] and r["stats"][9] >= 3


def test_the_named_cases_reach_every_branch():
    total = dict.fromkeys(lm.COUNTERS, 0)
    for name in NAMED:
        for c in model(name)["counters"]:
            for k in lm.COUNTERS:
                total[k] += 0 if c is None else c[k]
    assert all(total[k] > 0 for k in lm.COUNTERS), total
    first = {name: model(name)["counters"][0] for name in NAMED}
    assert first["noise25_invert_reject"]["invert"] and first["noise25_invert_reject"]["reject"] and first["noise25_invert_reject"]["r_lo"]
    assert first["noise25_invert"]["invert"] and not first["noise25_invert"]["reject"]
    assert first["translation_20"]["stop_r"] and model("translation_20")["S"][0][1] < 1e-20      # the data fit exactly
    assert first["inliers_64"]["r_hi"] and first["inliers_64"]["lambda_zero"] and first["inliers_64"]["stop_d"]
    for k in (1, 2):
        r = model("lm_iters_%d" % k)
        assert r["counters"][0]["stop_iter"] == 1 and r["stats"][8] == -k == r["stats"][10]      # negated at the limit (R:577-578)
    r = model("thresh2_above_inliers")
    assert r["stats"][0] == lm.ST_H and r["stats"][8] > 0 and r["stats"][10:].tolist() == [0, 0]
    assert [int(model("inliers_%d" % k)["stats"][1]) for k in (5, 6, 8, 9, 63, 64, 65)] == [5, 6, 8, 9, 63, 64, 65]


def test_lm_runs_after_a_refit_that_returned_0_and_never_for_4_rows():
    """R:668 ignores runKernel's result: where the refit over the inliers returns 0, LM starts from the RANSAC model.  n == 4 is R:641's branch."""
    four = cases.exact(4, 4)
    out = lm.find_homography2_lm(four[:, 0:2].copy(), four[:, 2:4].copy(), 3.0, 2000, 0.995, [])
    assert out.ok and out.lm == (0, 0) and out.counters is None
    real = hm.run_kernel
    calls = []

    def refit_fails(M, m):
        ok, H = real(M, m)
        calls.append(M.shape[1])
        if M.shape[1] > 4:                                            # the refit is the one call over more than four rows
            ok = np.zeros_like(ok)
        return ok, H
    pts = NAMED["inliers_9"][0]
    src, dst = pts[:, 0:2].copy(), pts[:, 2:4].copy()
    hm.run_kernel = refit_fails
    try:
        out = lm.find_homography2_lm(src, dst, 3.0, 2000, 0.995, [])
        plain = hm.find_homography2(src, dst, 3.0, 2000, 0.995, [])
    finally:
        hm.run_kernel = real
    assert 9 in calls and out.ok and out.lm[1] >= 3 and out.H[8] == plain.H[8]
    x, ret, nfJ, _, _ = lm.lm_run(plain.H[0:8], src, dst, 10)
    assert np.array_equal(out.H[:8], x) and out.lm == (ret, nfJ)


def test_header_arity_equals_the_ctypes_signature():
    from imagestitch_amd import _lib
    text = open(os.path.join(ROOT, "include", "imagestitch_hip.h"), encoding="utf-8").read()
    arity = {}
    for name in ("isx_find_homography_lm", "isx_find_homography"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert m, name
        arity[name] = len(m.group(1).split(","))
        assert arity[name] == len(_lib._SIGS[name]), (name, arity)
        assert name in _lib.declared_symbols()
    assert arity["isx_find_homography_lm"] == arity["isx_find_homography"] + 1 == 16
    i = [a.strip() for a in re.search(r"\bint\s+isx_find_homography_lm\s*\(([^;]*?)\)\s*;", text, re.S).group(1).split(",")]
    assert i[7] == "int num_matches_thresh2" and i[8] == "int lm_max_iters"


FUZZ_CASES = [(20261261783603, "tiny", "c0c79bfc13b233d7"), (20261261783604, "chunk_edges", "2d8e43dfb1eccec3"),
              (20261261783605, "count_limits", "591feb240cb8a34f"), (20261261783606, "noisy", "3fe91bef9febfbb2"),
              (20261261783607, "degenerate", "31104a48358b9bf7"), (20261261783608, "multi", "3b8c3edf7d6107a7")]


def test_the_fuzzers_cases_are_what_they_were():
    """Digests of case(seed, cls) recorded before --refine existed: the polish draws lm_max_iters from a generator of its own."""
    import fuzz_homography as f
    for seed, cls, want in FUZZ_CASES:
        c = f.case(seed, cls)
        h = hashlib.sha256()
        for p, n in c["pairs"]:
            h.update(p.tobytes())
            h.update(str((p.shape, int(n))).encode())
        h.update(json.dumps([sorted(c["kw"].items()), c["device"], c["wide"], c["spare"]]).encode())
        assert h.hexdigest()[:16] == want, (seed, cls)
    assert {f.lm_iters_of(s) for s in range(40)} == {1, 2, 10}


def test_the_cpp_wrapper_compiles_with_set_refine(tmp_path):
    import subprocess
    src = tmp_path / "refine.cpp"
    src.write_text('#include "imagestitch.hpp"\nint main() { isx::BestOf2NearestMatcher m(0.3f); m.setRefine(true); m.setRefine(true, 5);\n'
                   '    return (int)m.lmStats().size(); }\n')
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
