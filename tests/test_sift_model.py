"""tests/helpers/sift_np.py, the specification of isx_sift_find, against what SIFT must do whatever its arithmetic: its tables, the two
exponentials, the octave rule, blobs of known place and size, two orientation peaks, duplicates, the refinement's moves and its three
rejections, the order and the cap.  No GPU.  python tests/test_sift_model.py prints the records below."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pano_cases  # noqa: E402
import sift_cases as cases  # noqa: E402
from helpers import sift_np as M  # noqa: E402

# worst error in float32 ulps of the correctly rounded value over the arguments the finder can produce, 4 000 001 points each: the same
# figures stand in DESIGN.md §8 "Features finder, SIFT".  sift_math.hpp's class is "within one ulp".
MEASURED_ULP = {"expf": 0.49999983, "exp2f": 0.49999995}
SWEEPS = {"expf": (-32.0, 0.0, np.exp), "exp2f": (0.0, 2.0, np.exp2)}

# One blob of standard deviation s_b centred on source pixel (47.75, 47.75), per (octave, layer) of tests/sift_cases.py's BLOBS: what the model
# gives - the distance of pt from the centre in pixels (0.25 of it is OpenCV's own: pt is the doubled image's coordinate halved, which
# ignores the half-pixel phase of the doubling) and |size - 2 s_b| / (2 s_b) (the DoG extremum of a Gaussian blob lies at 0.89 s_b, not
# at s_b: size is near 1.77 s_b in every octave).  The bound is BOUND_FACTOR x the record.
RECORDED_BLOBS = {
    (-1, 1): (0.355, 0.129), (-1, 2): (0.354, 0.115), (-1, 3): (0.349, 0.114), (0, 1): (0.350, 0.112), (0, 2): (0.357, 0.110), (0, 3): (0.356, 0.110),
    (1, 1): (0.351, 0.111), (1, 2): (0.354, 0.109), (1, 3): (0.352, 0.109),
}


def test_tables_equal_their_formula():
    sig = M.sigmas()
    assert np.allclose(sig, [1.249, 1.2263, 1.5450, 1.9466, 2.4525, 3.0900], atol=5e-4)
    assert tuple(M.width_of(s) for s in sig) == M.WIDTHS == (11, 11, 13, 17, 21, 27) and sum(M.WIDTHS) == 100
    for got, want in zip(M.regenerate_taps(), M.TAPS):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert abs(float(want.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(want, want[::-1])


def test_the_header_holds_the_same_tables():
    """csrc/sift_tables.hpp's hexadecimal literals are the model's bits, its widths and offsets the model's"""
    text = open(os.path.join(ROOT, "imagestitch_amd", "csrc", "sift_tables.hpp")).read()
    body = text[text.index("float sift_tap("):]
    body = body[body.index("{", body.index("const float t[")) + 1:body.index("};")]
    lines = [ln for ln in body.splitlines() if not ln.strip().startswith("//")]
    got = np.array([float.fromhex(v.strip().rstrip("f")) for v in " ".join(lines).split(",") if v.strip()], np.float64)
    want = np.concatenate(M.TAPS)
    assert len(got) == 100 and np.array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32)) and np.array_equal(got, want.astype(np.float64))
    for name, values in (("sift_tap_width", M.WIDTHS), ("sift_tap_first", tuple(int(v) for v in np.cumsum((0,) + M.WIDTHS[:-1])))):
        b = text[text.index("int " + name):]
        assert tuple(int(v) for v in b[b.index("{", b.index("[SIFT_KERNELS]")) + 1:b.index("};")].split(",")) == values, name


def test_exponentials_within_one_ulp():
    """pm_expf on [-32, 0] and pm_exp2f on [0, 2], densely, against float64 rounded to float32: the measured worst error, and the class"""
    for name, (lo, hi, fn) in SWEEPS.items():
        x = np.linspace(lo, hi, 4_000_001).astype(np.float32)
        worst = float(M.ulp_error(getattr(M, name)(x), x, fn).max())
        print(name, "worst ulp error", worst)
        assert worst <= 1.0, (name, worst)
        assert abs(worst - MEASURED_ULP[name]) < 5e-7, (name, worst)
    assert M.expf(np.float32(0)) == 1 and M.exp2f(np.float32(1)) == 2 and M.exp2f(np.float32(-3)) == 0.125
    with np.errstate(all="ignore"):
        edge = M.expf(np.array([np.nan, 89.5, -104.5, np.inf, -np.inf], np.float32))
    assert np.isnan(edge[0]) and edge[1] == np.inf and edge[2] == 0 and edge[3] == np.inf and edge[4] == 0


def test_octave_rule_in_integers():
    for m in range(1, 16385):
        assert M.octave_count(m) == max(int(np.rint(np.log2(np.float64(m)) - 2.0)) + 1, 0), m
    assert M.octave_sizes(5, 5) == [] and M.octave_sizes(6, 6) == [(12, 12)] and M.octave_sizes(33, 47) == [(66, 94), (33, 47), (16, 23)]
    assert M.octave_sizes(6, 200) == [(12, 400)] and M.octave_sizes(240, 320)[-1] == (15, 20)


def test_reflection_repeats():
    assert M.reflect101(np.arange(-13, 25), 12).tolist() == [abs((p + 11) % 22 - 11) for p in range(-13, 25)]
    assert M.reflect101(np.arange(-5, 5), 1).tolist() == [0] * 10 and M.reflect101(np.arange(-5, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    flat = M.blur(np.full((3, 4), 7, np.float32), M.TAPS[5])
    assert flat.shape == (3, 4) and np.abs(flat - 7).max() < 1e-5


def test_sum_in_order_is_sequential():
    rng = np.random.default_rng(3)
    bins, vals = rng.integers(0, 7, 500), (rng.normal(0, 1, 500) * 10.0 ** rng.integers(-3, 4, 500)).astype(np.float32)
    want = np.zeros(7, np.float32)
    for b, v in zip(bins, vals):
        want[b] = np.float32(want[b] + v)
    assert np.array_equal(M.sum_in_order(7, bins, vals), want)


def _blob_record(key):
    r, t = cases.traced("blob-%d-%d" % key)
    c = t["candidates"]
    s_b = cases.BLOBS[key]
    centre = float(np.hypot(*(r["keypoints"][0] - 47.75)))
    return r, c, centre, abs(float(r["meta"][0, 0]) - 2 * s_b) / (2 * s_b)


def test_one_blob_one_candidate_at_its_centre_and_scale():
    """Ground truth: a blob of standard deviation s_b gives ONE candidate, in the planned layer of the planned octave, at the blob's centre
    and of a size near 2 s_b.  (An isotropic blob has no dominant direction: how many peaks its orientation histogram shows is chance, so
    the candidate is counted, and every keypoint of it has its pt and size.)"""
    for key in sorted(cases.BLOBS):
        r, c, centre, size = _blob_record(key)
        print(key, "centre error %.3f px, size error %.3f" % (centre, size), "keypoints", r["count"])
        assert len(c["octave"]) == 1 and (int(c["octave"][0]) - 1, int(c["layer"][0])) == key, key
        assert r["count"] >= 1 and (r["keypoints"] == r["keypoints"][0]).all() and (r["meta"][:, [0, 2, 3, 4]] == r["meta"][0, [0, 2, 3, 4]]).all()
        assert (r["meta"][0, 3], r["meta"][0, 4]) == key
        assert centre <= pano_cases.BOUND_FACTOR * RECORDED_BLOBS[key][0] and size <= pano_cases.BOUND_FACTOR * RECORDED_BLOBS[key][1], (key, centre, size)


def test_a_dark_blob_gives_the_same_keypoint():
    bright, dark = cases.want("blob-0-2"), cases.want("blob-dark")
    assert dark["count"] >= 1 and np.abs(dark["keypoints"][0] - bright["keypoints"][0]).max() < 0.02
    assert abs(float(dark["meta"][0, 0] - bright["meta"][0, 0])) < 0.05 and (dark["meta"][0, 3:] == bright["meta"][0, 3:]).all()


def test_two_lobes_two_keypoints_from_one_candidate():
    r, t = cases.traced("two-lobes")
    assert len(t["candidates"]["octave"]) == 1 and t["peaks"] == [2] and r["count"] == 2
    assert (r["keypoints"][0] == r["keypoints"][1]).all() and r["meta"][0, 0] == r["meta"][1, 0]
    a = r["meta"][:, 1]
    assert a[0] > a[1] and abs(abs(float(a[0] - a[1])) - 180) < 1.0          # ascending bin is descending angle (angle = 360 - 10 bin)
    assert not np.array_equal(r["descriptors"][0], r["descriptors"][1])


def test_duplicates_are_removed():
    r, t = cases.traced("duplicates")
    assert t["counters"]["duplicates"] >= 1
    c = t["candidates"]
    keys = list(zip(c["octave"].tolist(), c["layer"].tolist(), c["r"].tolist(), c["c"].tolist()))
    assert len(set(keys)) == len(keys) == sum(1 for p in t["peaks"] if p >= 0)


def test_refinement_moves_and_rejects():
    """a candidate that changes layer, one that changes pixel, and each of the three rejections, across the cases"""
    total = M.new_counters()
    for name in ("odd-33x47", "contrast-0", "rig-gray", "straight-edge"):
        for k, v in cases.traced(name)[1]["counters"].items():
            total[k] += v
    print(total)
    assert total["moved_layer"] >= 1 and total["moved_pixel"] >= 1
    assert total["rej_contrast"] >= 1 and total["rej_edge"] >= 1 and total["rej_steps"] >= 1 and total["rej_left"] >= 1
    edge = cases.traced("straight-edge")
    assert edge[0]["count"] == 0 and edge[1]["counters"]["extrema"] > 0 and edge[1]["counters"]["rej_edge"] == edge[1]["counters"]["extrema"]
    assert cases.want("flat")["count"] == 0 and cases.want("contrast-huge")["count"] == 0


def _key(meta, kp):
    return [(-float(m[2]), -float(m[0]), -float(m[3]), -float(k[1]), -float(k[0])) for m, k in zip(meta, kp)]


def test_output_order_and_values():
    for name in ("rig-gray", "contrast-0", "odd-33x47"):
        r = cases.want(name)
        k = _key(r["meta"], r["keypoints"])
        assert k == sorted(k), name
        d = r["descriptors"]
        assert d.shape[1] == 128 and (d == np.rint(d)).all() and d.min() >= 0 and d.max() <= 255
        assert (r["meta"][:, 1] >= 0).all() and (r["meta"][:, 1] < 360).all() and (r["meta"][:, 3] >= -1).all()
    C = dict(response=np.float32([4, 5, 4, 4]), size=np.float32([15, 21, 15, 15]), octave=np.array([0, 0, 0, 0]), y=np.float32([6, 9, 6, 7]), x=np.float32([5, 9, 5, 5]))
    assert M.order(C).tolist() == [1, 3, 0, 2]


def test_cap_and_nfeatures_keep_a_prefix():
    whole = cases.want("rig-gray")
    n = whole["count"]
    for cap in (1, 17, n - 1, n, n + 1):
        r = cases.want("rig-gray", cap)
        assert r["count"] == min(cap, n) and r["status"] == (M.STATUS_TRUNCATED if cap < n else 0), cap
        for k in ("keypoints", "meta", "descriptors"):
            assert np.array_equal(r[k], whole[k][:cap]), (cap, k)
    for nf in (1, n - 1, n, n + 1):
        r = cases.want("rig-gray", None, nf)
        assert r["count"] == min(nf, n) and r["status"] == 0 and np.array_equal(r["descriptors"], whole["descriptors"][:nf]), nf


def test_channels_agree():
    """gray is one rule for 1, 3 and 4 channels: a view and its gray version give the same keypoints"""
    v = cases.rig_view(1, 3)
    a, b = M.find(v), cases.want("rig-gray")
    assert a["count"] == b["count"] and np.array_equal(a["descriptors"], b["descriptors"])


if __name__ == "__main__":
    for key in sorted(cases.BLOBS):
        r, c, centre, size = _blob_record(key)
        print(key, "(%.3f, %.3f)," % (centre, size), r["count"], [(int(o) - 1, int(l)) for o, l in zip(c["octave"], c["layer"])])
    for name, (lo, hi, fn) in SWEEPS.items():
        x = np.linspace(lo, hi, 4_000_001).astype(np.float32)
        print(name, "%.8f" % float(M.ulp_error(getattr(M, name)(x), x, fn).max()))
