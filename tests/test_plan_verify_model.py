"""The three-valued model of the planned-ROI verification (tests/helpers/plan_verify_np.py) and the fixed cameras it is applied to
(tests/plan_verify_cases.py), on the CPU: known answers for the stand-ins and the truncation intervals, every class present and every case
of its class, every true plan MUST_PASS, the share of shifted plans the model makes no claim about under the cap - so that the GPU tests
(tests/test_gpu_plan_verify.py) cannot hide a miss behind plans nobody asserts on - and the model's verdict on the stale plans the verifier
accepted before this suite."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_verify_cases as PC  # noqa: E402
from helpers import plan_verify_np as M  # noqa: E402


def test_diamond_angle_known_answers():
    s = 100.0
    for u, d in [(0.0, 0.0), (s * math.pi / 4, 0.5), (s * math.pi / 2, 1.0), (s * 3 * math.pi / 4, 1.5), (s * math.pi, 2.0),
                 (-s * math.pi / 4, -0.5), (-s * math.pi / 2, -1.0), (-s * 3 * math.pi / 4, -1.5), (-s * math.pi, -2.0)]:
        assert M.d_of_u(u, s) == pytest.approx(d, abs=1e-12), u
    # the two branches: t before a right angle, 2 - t past it; tan(theta) = 1/2 and its supplement
    th = math.atan(0.5)
    assert M.d_of_u(s * th, s) == pytest.approx(1.0 / 3.0, abs=1e-12)
    assert M.d_of_u(s * (math.pi - th), s) == pytest.approx(2.0 - 1.0 / 3.0, abs=1e-12)
    assert M.d_of_u(-s * (math.pi - th), s) == pytest.approx(-(2.0 - 1.0 / 3.0), abs=1e-12)
    # clamped at +-pi: what lies beyond is the seam itself
    assert M.d_of_u(s * math.pi + 1.0, s) == pytest.approx(2.0, abs=1e-12) and M.d_of_u(-s * math.pi - 50.0, s) == pytest.approx(-2.0, abs=1e-12)
    us = np.linspace(-s * math.pi, s * math.pi, 2001)
    ds = [M.d_of_u(u, s) for u in us]
    assert all(b > a for a, b in zip(ds, ds[1:])), "strictly increasing on [-pi scale, pi scale]"


def test_q_and_w_known_answers():
    assert M.q_of_v(-37.5, 75.0) == -0.5 and M.q_of_v(0.0, 3.0) == 0.0
    s = 50.0
    for v, w in [(0.0, -1.0), (s * math.pi / 3, -0.5), (s * math.pi / 2, 0.0), (s * 2 * math.pi / 3, 0.5), (s * math.pi, 1.0)]:
        assert M.w_of_v(v, s) == pytest.approx(w, abs=1e-12), v
    assert M.w_of_v(-1.0, s) == -1.0 and M.w_of_v(s * math.pi + 1.0, s) == 1.0          # clamped at the poles
    ws = [M.w_of_v(v, s) for v in np.linspace(0.0, s * math.pi, 1001)]
    assert all(b > a for a, b in zip(ws, ws[1:]))


def test_trunc_interval_three_cases():
    assert M.trunc_interval(-7) == (-8.0, -7.0)
    assert M.trunc_interval(0) == (-1.0, 1.0)
    assert M.trunc_interval(12) == (12.0, 13.0)
    for x in (-7.999, -7.0, -0.999, 0.0, 0.999, 12.0, 12.999):
        lo, hi = M.trunc_interval(int(x))
        assert lo <= x <= hi


def test_bound_verdict_three_values():
    s = 100.0          # cylindrical v: q = v / 100, t = 8e-6 in q = 8e-4 px
    assert M.bound_verdict(M.CYL, s, 1, 12, 12.5) == M.MUST_PASS
    assert M.bound_verdict(M.CYL, s, 1, 12, 13.5) == M.MUST_FLAG and M.bound_verdict(M.CYL, s, 1, 12, 11.5) == M.MUST_FLAG
    assert M.bound_verdict(M.CYL, s, 1, 12, 12.0004) == M.NO_CLAIM and M.bound_verdict(M.CYL, s, 1, 12, 11.9996) == M.NO_CLAIM
    assert M.bound_verdict(M.CYL, s, 1, 12, 12.0012) == M.MUST_PASS and M.bound_verdict(M.CYL, s, 1, 12, 11.9988) == M.MUST_FLAG
    assert M.bound_verdict(M.CYL, s, 3, -3, -3.5) == M.MUST_PASS and M.bound_verdict(M.CYL, s, 3, -3, -2.5) == M.MUST_FLAG
    assert M.bound_verdict(M.CYL, s, 0, 0, -0.9) == M.MUST_PASS and M.bound_verdict(M.CYL, s, 0, 0, 0.9) == M.MUST_PASS
    assert M.bound_verdict(M.CYL, s, 0, 0, -1.1) == M.MUST_FLAG and M.bound_verdict(M.CYL, s, 0, 0, 1.1) == M.MUST_FLAG


def test_every_class_and_required_size_is_present():
    assert sorted({c[0] for c in PC.CASES}) == sorted(PC.CLASSES)
    assert 55 <= len(PC.CASES) <= 80
    sizes = {(c[2], c[3]) for c in PC.CASES}
    assert all(s in sizes for s in PC.REQUIRED_SIZES), sizes
    for size in [(256, 128), (257, 129)]:          # one and two scan blocks each way: through the full scan, not only the border's
        assert any((c[2], c[3]) == size and c[0] in ("cyl_corner_behind", "cyl_rolled", "cyl_straddle") for c in PC.CASES), size
    for c in PC.CASES:
        assert 0.5 <= c[7] / c[4] <= 2.0, c
    assert len({PC.case_id(c) for c in PC.CASES}) == len(PC.CASES)


@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=[PC.case_id(c) for c in PC.CASES])
def test_every_case_is_of_its_class(oracle, i):
    case = PC.CASES[i]
    cls = case[0]
    kind, scale, K, R, w, h = PC.camera(case)
    t = PC.truth(oracle, i)
    roi, (scan, why) = t["roi"], t["scan"]
    lim = M.f2i(np.float32(scale) * np.float32(M.PI_F))
    assert t["verdicts"][0][0] == M.MUST_PASS, (cls, roi, t["extrema"], t["verdicts"][0])
    assert all(math.isfinite(e) for e in t["extrema"])
    if cls.startswith("cyl_"):
        assert kind == M.CYL
    if cls.startswith("sph_"):
        assert kind == M.SPH and scan == "roi_border_sph"
    if cls == "cyl_light":
        assert scan == "roi_border"
    if cls == "cyl_corner_behind":
        assert (scan, why) == ("roi_scan", "corner_behind")
    if cls == "cyl_pole":
        assert (scan, why) == ("roi_scan", "cyl_pole")
    if cls == "cyl_pole_inside":
        north, south = M.sph_poles(K, R, w, h)      # (the same arithmetic projects the cylinder's axis)
        assert scan == "roi_scan" and (north or south) and roi[0] == -lim and roi[2] == lim
    if cls == "cyl_rolled":
        assert (scan, why) == ("roi_scan", "rolled") and abs(case[10]) > math.pi / 2
    if cls == "sph_plain":
        assert not t["north"] and not t["south"]
    if cls == "sph_north":
        assert t["north"] and not t["south"] and roi[3] == M.f2i(np.float32(math.pi * scale))
    if cls == "sph_south":
        assert t["south"] and not t["north"] and roi[1] == 0
    if cls.endswith("_on_seam"):
        assert roi[2] == lim and t["extrema"][2] == float(np.float32(scale) * np.float32(M.PI_F))
    if cls in ("sph_north_edge", "sph_south_edge"):
        # the border's own extremum in v, before the pole replaces it (top and bottom rows: the pole lies beside one of them)
        _, _, r_kinv, _ = oracle.camera(K, R)
        vs = [float(oracle.map_forward(kind, scale, r_kinv, float(x), float(y))[1]) for x in range(w) for y in (0, h - 1)]
        if cls == "sph_north_edge":
            assert t["north"] and not t["south"] and M.f2i(max(vs)) == roi[3] - 1
        else:
            assert t["south"] and not t["north"] and M.f2i(min(vs)) == 1
    if cls == "sph_pole_one_sided":
        _, _, r_kinv, _ = oracle.camera(K, R)
        pts = [(x, y) for x in range(w) for y in (0, h - 1)] + [(x, y) for y in range(h) for x in (0, w - 1)]
        us = [float(oracle.map_forward(kind, scale, r_kinv, float(x), float(y))[0]) for x, y in pts]
        assert (t["north"] or t["south"]) and roi[0] == 0 and min(us) >= 1.0       # the border alone would give tl.u >= 1
    if cls.endswith("_straddle"):
        assert roi[0] <= -lim + 1 and roi[2] >= lim - 1 and not t["north"] and not t["south"]
    if cls == "zero_bound":
        assert 0 in roi and np.array_equal(R, np.eye(3, dtype=np.float32))
    if cls == "all_negative":
        assert max(roi) < 0
    if cls == "all_positive":
        assert min(roi) > 0


def test_zero_bound_from_both_sides(oracle):
    """a bound that truncates to 0 from below (-1 < extremum < 0) and from above (0 < extremum < 1)"""
    signs = set()
    for i, c in enumerate(PC.CASES):
        if c[0] == "zero_bound":
            t = PC.truth(oracle, i)
            signs |= {math.copysign(1.0, e) for e, r in zip(t["extrema"], t["roi"]) if r == 0 and e != 0.0}
    assert signs == {-1.0, 1.0}


def test_no_claim_share_is_under_the_cap(oracle):
    counts = {M.MUST_PASS: 0, M.NO_CLAIM: 0, M.MUST_FLAG: 0}
    rules = {}
    for i in range(len(PC.CASES)):
        for v, per in PC.truth(oracle, i)["verdicts"][1:]:
            counts[v] += 1
            if v == M.MUST_FLAG and len(per) == 1:
                rules[per[0]] = rules.get(per[0], 0) + 1
    n = sum(counts.values())
    print(counts, rules)
    assert n == 8 * len(PC.CASES)
    assert counts[M.NO_CLAIM] <= PC.NO_CLAIM_CAP * n, counts
    assert counts[M.MUST_FLAG] >= 0.8 * n, counts
    assert all(rules.get(r, 0) >= 4 for r in ("u_beyond_pi", "north_pole", "south_pole")), rules


def test_model_flags_the_stale_plans_the_verifier_used_to_accept():
    # a north pole inside a 129 x 46 source, scale 73.6: the ROI is [-223 189 222 231], br.v = (int)(pi scale) is the pole's; 230 is not
    ex = [-223.4, 189.5, 222.6, float(np.float32(math.pi * 73.6))]
    assert M.f2i(ex[3]) == 231
    assert M.verdict(M.SPH, 73.6, [-223, 189, 222, 231], ex, north=True)[0] == M.MUST_PASS
    assert M.verdict(M.SPH, 73.6, [-223, 189, 222, 230], ex, north=True) == (M.MUST_FLAG, ["north_pole"])
    assert M.verdict(M.SPH, 73.6, [-223, 189, 222, 232], ex, north=True) == (M.MUST_FLAG, ["north_pole"])
    # without the pole the same border extremum decides: 230.6 lies in [230, 231)
    assert M.verdict(M.SPH, 73.6, [-223, 189, 222, 230], ex[:3] + [230.6])[0] == M.MUST_PASS
    # the south pole dictates tl.v = 0
    assert M.verdict(M.SPH, 73.6, [-223, 1, 222, 40], [-223.4, 0.0, 222.6, 40.5], south=True) == (M.MUST_FLAG, ["south_pole"])
    # cylindrical, 179 x 150, scale 70.8: (int)(70.8 pi_f) = 222, the tile straddles the back seam with tl.u = -222; -223 is unattainable
    assert M.f2i(np.float32(70.8) * np.float32(M.PI_F)) == 222
    ex = [-222.2, -40.3, 222.3, 55.6]
    assert M.verdict(M.CYL, 70.8, [-222, -40, 222, 55], ex)[0] == M.MUST_PASS
    assert M.verdict(M.CYL, 70.8, [-223, -40, 222, 55], ex) == (M.MUST_FLAG, ["u_beyond_pi"])
    assert M.verdict(M.CYL, 70.8, [-222, -40, 223, 55], ex) == (M.MUST_FLAG, ["u_beyond_pi"])
    # the documented blind zone near a spherical pole: scale 617, tl.v = 1.81 against a planned 0 is 3e-6 away in w = -cos(v / scale)
    assert M.bound_verdict(M.SPH, 617.0, 1, 0, 1.81) == M.NO_CLAIM
    assert M.bound_verdict(M.SPH, 617.0, 1, 0, 4.0) == M.MUST_FLAG
