"""The argument sweeps over which imagestitch_amd/csrc/bundle_math.hpp is held to one answer by three parties: the Python model
(tests/helpers/bundle_np.py, bundle_reproj_np.py), the host compilation (isx_selftest_bundle_math) and the device compilation
(isx_selftest_bundle_math_device).  tests/test_gpu_bundle_math.py compares the three by bits; tests/test_bundle_model.py holds the model's
sin, cos, acos and Rodrigues round trip over the same sweeps to mpmath.  sweeps() -> {name: (fn, rows of inputs, columns out)}; model(name,
rows) -> the model's outputs as rows of float64.  Every sweep aims at a branch or a threshold of the header:
  sin, cos     the quadrant switches of bm_reduce (both neighbours of every multiple of pi / 4 up to 4 pi), all four quadrants, +-0, a
               denormal-range argument, 2^51 + 1 (meaningless, but the same everywhere), +-inf and NaN;
  acos         the three branches either side of +-0.5, the ends +-1 with the neighbours outside [-1, 1] (NaN), 0 and 1 - 2^-53;
  rodrigues    vector -> matrix either side of DBL_EPSILON and at a quarter, half, three-quarter (quadrant -1) and full turn; matrix ->
               vector on those, on exact half turns with every sign case of its tie-break line, the identity, and s either side of 1e-5
               for both signs of c;
  polar        rotations scaled as the estimator leaves them, their mirror images (det < 0), a singular, an infinite and the zero matrix;
  jacobi       the moment matrices of the wave rigs, diagonal matrices, a double eigenvalue, an off-diagonal at the threshold and just
               above it, in float64 and in float32;
  cam_h, ray, reproj_h, reproj_err
               the parameters, keypoints and edges of the rigs that go round (bundle_cases.WIDE), and a Z of 0."""
import functools
import math

import numpy as np

import bundle_cases as bc
import bundle_reproj_cases as rc
from helpers import bundle_np as bm
from helpers import bundle_reproj_np as rp
from helpers.homography_lm_np import jacobi_n

PI = math.pi
FN = dict(sin=0, cos=1, acos=2, rodrigues_mat=3, rodrigues_vec=4, polar=5, cam_h=6, ray=7, jacobi3f=8, jacobi3=9, reproj_h=10, reproj_err=11)
N_OUT = dict(sin=1, cos=1, acos=1, rodrigues_mat=9, rodrigues_vec=3, polar=10, cam_h=9, ray=3, jacobi3f=12, jacobi3=12, reproj_h=9, reproj_err=2)
WIDE_RIGS = ("ring_8x45_center_0", "ring_8x45_center_4", "ring_8x45_exact_half_turn", "arc_5x50_natural_end")


def _both(v):
    """v with both neighbours of each of its values."""
    v = np.asarray(v, np.float64)
    return np.concatenate([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


def angles():
    return np.concatenate([np.linspace(-4 * PI, 4 * PI, 20001), _both(np.arange(-16, 17) * (PI / 4)),
                           [0.0, -0.0, 1e-300, -1e-300, 2.0 ** 51 + 1, -(2.0 ** 51 + 1), np.inf, -np.inf, np.nan]])


def cosines():
    return np.concatenate([np.linspace(-1.0, 1.0, 20001), _both([0.5, -0.5, 1.0, -1.0]), [0.0, -0.0, 1.0 - 2.0 ** -53]])


def _axes():
    rng = np.random.default_rng(41)
    a = rng.normal(size=(6, 3))
    return np.concatenate([a / np.linalg.norm(a, axis=1, keepdims=True), np.eye(3), -np.eye(3)[:1]])


def rotation_vectors():
    lengths = np.concatenate([_both([PI / 4, PI / 2, PI, 3 * PI / 2]), [2 * PI, 0.1, 1.0, 3.0]])
    rows = [a * t for a in _axes() for t in lengths]
    eps = bm.DBL_EPSILON
    rows += [np.zeros(3), [eps * 0.5, 0, 0], [0, np.nextafter(eps, 0), 0], [0, 0, eps], [np.nextafter(eps, 1), 0, 0], [1e-16, 1e-16, 1e-16],
             [1.3e-16, 1.3e-16, 1.3e-16], [3e-16, 0, 0], [1e-9, -1e-9, 1e-9]]
    return np.array([np.asarray(r, np.float64) for r in rows])


def _half_turn(axis):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return (2.0 * np.outer(a, a) - np.eye(3)).ravel()


def _small_s_of(R):
    """s of bm_rodrigues_vec in the model's arithmetic."""
    rx, ry, rz = R[7] - R[5], R[2] - R[6], R[3] - R[1]
    return math.sqrt((((rx * rx) + (ry * ry)) + (rz * rz)) * 0.25)


def rotation_matrices():
    rows = [np.array(bm.rodrigues_mat([float(v) for v in rv])) for rv in rotation_vectors()]
    # exact half turns: the axes, (1, 1, 0) / sqrt 2, and rx the smallest with every sign of ry, rz (the tie-break line negates rz or not)
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 0], [0, 1, 1], [0, 1, -1], [1, 0, 1], [0, -2, 1], [0, 3, -1], [0.1, 0.7, 0.7], [0.1, -0.7, 0.7], [0.1, 0.7, -0.7],
                 [0.1, -0.7, -0.7], [-0.1, 0.7, 0.7], [-0.1, -0.7, 0.7], [0.7, 0.1, 0.7], [0.7, 0.7, -0.1], [0.7, -0.1, -0.7]):
        rows.append(_half_turn(axis))
    rows.append(np.eye(3).ravel())
    # s either side of 1e-5 for c > 0 (an angle near 1e-5) and c < 0 (near pi - 1e-5)
    for base in (0.0, PI):
        for f in (1.0 - 1e-6, 1.0 - 1e-9, 1.0 - 1e-12, 1.0, 1.0 + 1e-12, 1.0 + 1e-9, 1.0 + 1e-6):
            t = abs(base - 1e-5 * f)
            for a in _axes()[5:8]:
                rows.append(np.array(bm.rodrigues_mat([float(v) for v in a * t])))
    return np.array(rows)


def polar_inputs():
    rng = np.random.default_rng(42)
    rows = []
    for k in range(24):
        R = bc.rotation(*rng.uniform(-PI, PI, 3)) * 1.02 ** (k % 3)
        R = R.astype(np.float32).astype(np.float64)            # the adjuster reads the estimator's R as float32
        rows += [R.ravel(), (R @ np.diag([1.0, 1.0, -1.0])).ravel()]
    rows += [np.array([1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 1.0, 1.0]), np.array([1.0, 0, 0, 0, np.inf, 0, 0, 0, 1.0]), np.zeros(9), np.full(9, np.nan),
             np.diag([1e200, 1.0, 1.0]).ravel()]
    return np.array(rows)


def _moment32(cams):
    """The float32 moment matrix of the wave correction: the sum of x x^T over the cameras' first columns."""
    T = np.float32
    m = [T(0)] * 9
    for R in cams[:, 4:13]:
        R = [T(v) for v in R]
        col = (R[0], R[3], R[6])
        for r in range(3):
            for q in range(3):
                m[3 * r + q] = m[3 * r + q] + (col[r] * col[q])
    return np.array(m, np.float64)


def symmetric_matrices(eps):
    """9 doubles a row; eps: the threshold of the Jacobi that will read them."""
    rows = [_moment32(c) for _, c in sorted(rc.wave_rigs().items())]
    rows += [np.diag(d).ravel() for d in ([3.0, 2.0, 1.0], [1.0, 2.0, 3.0], [2.0, 2.0, 2.0], [0.0, 0.0, 0.0], [1.0, -1.0, 0.5])]
    u = np.array([1.0, 2.0, 2.0]) / 3.0
    rows += [(np.eye(3) + np.outer(u, u)).ravel(), (2.0 * np.eye(3) - np.outer(u, u)).ravel()]      # eigenvalues 2, 1, 1 and 2, 2, 1
    for v in (eps, float(np.nextafter(np.float32(eps), np.float32(1))) if eps > 1e-10 else float(np.nextafter(eps, 1.0)), -eps):
        for at in (1, 2, 5):
            a = np.diag([3.0, 2.0, 1.0]).ravel()
            a[at] = v                                          # the upper triangle is what is read
            rows.append(a)
    rng = np.random.default_rng(43)
    for _ in range(12):
        m = rng.normal(size=(3, 3))
        rows.append((m @ m.T).ravel())
    return np.array(rows).astype(np.float32).astype(np.float64) if eps > 1e-10 else np.array(rows)


@functools.lru_cache(maxsize=None)
def _wide_params():
    """Per rig of WIDE_RIGS: (case, Ray's parameters after one iteration, Reproj's)."""
    ray, reproj = bc.named(), rc.named()
    out = []
    for name in WIDE_RIGS:
        c, d = ray[name], reproj[name]
        a = bm.adjust_rig(c["sizes"], c["keypoints"], c["pairs"], c["matches"], c["masks"], c["counts"][0], c["conf"][0], c["est_rig_stats"][0],
                          c["cameras_in"], max_iter=1)
        b = rp.adjust_rig(d["sizes"], d["keypoints"], d["pairs"], d["matches"], d["masks"], d["counts"][0], d["conf"][0], d["est_rig_stats"][0],
                          d["cameras_in"], max_iter=1)
        out.append((c, a["param"], d, b["param"]))
    return out


def camera_rows():
    """f, rvec[3], width, height of every camera of the wide rigs."""
    return np.array([p[4 * i:4 * i + 4] + [float(c["sizes"][i][0]), float(c["sizes"][i][1])] for c, p, _, _ in _wide_params() for i in range(len(c["sizes"]))])


def ray_rows():
    """H[9], x, y: R K^-1 of every camera of the wide rigs on its first keypoints; then a third row of zeros (Z = 0) and a zero matrix."""
    rows = []
    for c, p, _, _ in _wide_params():
        for i in range(len(c["sizes"])):
            H = bm.cam_h(p[4 * i:4 * i + 4], *c["sizes"][i])
            rows += [H + [float(x), float(y)] for x, y in c["keypoints"][i][:6]]
    H = list(rows[0][:6]) + [0.0, 0.0, 0.0]
    rows += [H + [100.0, 200.0], [0.0] * 9 + [1.0, 2.0], H[:2] + [0.0] * 7 + [0.0, 5.0]]
    return np.array(rows)


def edge_rows():
    """The seven parameters of both cameras of every edge of the wide rigs."""
    return np.array([p[7 * i:7 * i + 7] + p[7 * j:7 * j + 7] for _, _, d, p in _wide_params() for i, j in d["pairs"]])


def reproj_err_rows():
    """H[9], x1, y1, x2, y2: the edge matrix of every edge of the wide rigs on its first matches; then Z = 0 (a third row of zeros: x / 0 and
    0 / 0) and a Z that cancels to zero."""
    rows = []
    for _, _, d, p in _wide_params():
        for k, (i, j) in enumerate(d["pairs"]):
            H = rp.edge_h(p[7 * i:7 * i + 7], p[7 * j:7 * j + 7])
            for q, t, _ in d["matches"][k][:4]:
                rows.append(H + [float(v) for v in d["keypoints"][i][q]] + [float(v) for v in d["keypoints"][j][t]])
    H = list(rows[0][:6])
    rows += [H + [0.0, 0.0, 0.0] + [10.0, 20.0, 30.0, 40.0], [0.0] * 9 + [1.0, 2.0, 3.0, 4.0], H + [1.0, 0.0, -8.0] + [8.0, 3.0, 1.0, 1.0]]
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def sweeps():
    """name -> the rows of inputs (a 2-D float64 array, read-only)."""
    out = dict(sin=angles().reshape(-1, 1), cos=angles().reshape(-1, 1), acos=cosines().reshape(-1, 1), rodrigues_mat=rotation_vectors(),
               rodrigues_vec=rotation_matrices(), polar=polar_inputs(), cam_h=camera_rows(), ray=ray_rows(), jacobi3f=symmetric_matrices(float(rp.FLT_EPSILON)),
               jacobi3=symmetric_matrices(bm.DBL_EPSILON), reproj_h=edge_rows(), reproj_err=reproj_err_rows())
    for a in out.values():
        a.setflags(write=False)
    return out


def _jacobi3(row):
    W, V, _ = jacobi_n(row, 3)
    return [v for r in V for v in r] + list(W)


def _jacobi3f(row):
    W, V = rp.jacobi3_f32(row)
    return [float(v) for r in V for v in r] + [float(w) for w in W]


def _polar(row):
    Q, ok = bm.polar(row)
    return Q + [1.0 if ok else 0.0]


_MODEL = dict(sin=lambda r: [bm.sin(r[0])], cos=lambda r: [bm.cos(r[0])], acos=lambda r: [bm.acos(r[0])], rodrigues_mat=bm.rodrigues_mat,
              rodrigues_vec=bm.rodrigues_vec, polar=_polar, cam_h=lambda r: bm.cam_h(r[:4], int(r[4]), int(r[5])), ray=lambda r: bm.ray(r[:9], r[9], r[10]),
              jacobi3f=_jacobi3f, jacobi3=_jacobi3, reproj_h=lambda r: rp.edge_h(r[:7], r[7:14]), reproj_err=lambda r: rp.reproj_err(r[:9], r[9], r[10], r[11], r[12]))


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's outputs over sweeps()[name]: rows of float64."""
    with np.errstate(all="ignore"):
        out = np.array([list(_MODEL[name]([float(v) for v in row])) for row in sweeps()[name]], np.float64).reshape(-1, N_OUT[name])
    out.setflags(write=False)
    return out


class BranchCounter:
    """Counts, while a model runs, the branches of bundle_math.hpp that depend on how far a rig turns: wraps _reduce, acos, rodrigues_vec and
    polar of tests/helpers/bundle_np.py (and the names bundle_reproj_np.py imported from it) for the length of a `with`.  taken: {branch:
    times}; the branches: "quadrant -2" .. "quadrant 2", "acos mid" (|x| < 0.5), "acos neg" (x <= -0.5), "acos pos", "half turn" (s < 1e-5,
    c <= 0), "identity" (s < 1e-5, c > 0), "det < 0" (the polar factor negated)."""
    NAMES = ["quadrant %d" % q for q in (-2, -1, 0, 1, 2)] + ["acos mid", "acos neg", "acos pos", "half turn", "identity", "det < 0"]

    def __init__(self):
        self.taken = {k: 0 for k in self.NAMES}
        self._saved = []

    def __enter__(self):
        taken = self.taken
        reduce_, acos_, vec_, polar_ = bm._reduce, bm.acos, bm.rodrigues_vec, bm.polar

        def _reduce(x):
            r, q = reduce_(x)
            if q == q:
                taken["quadrant %d" % int(q)] += 1
            return r, q

        def acos(x):
            taken["acos mid" if (x < 0.5 and x > -0.5) else ("acos neg" if x < 0.0 else "acos pos")] += 1
            return acos_(x)

        def rodrigues_vec(R):
            if _small_s_of(R) < 1e-5:
                taken["identity" if (((R[0] + R[4]) + R[8]) - 1.0) * 0.5 > 0 else "half turn"] += 1
            return vec_(R)

        def polar(R):
            Q, ok = polar_(R)
            if ok and np.linalg.det(np.array(R).reshape(3, 3)) < 0:      # Q = R M with M positive definite: det Q has the sign of det R
                taken["det < 0"] += 1
            return Q, ok

        for mod, name, fn in ((bm, "_reduce", _reduce), (bm, "acos", acos), (bm, "rodrigues_vec", rodrigues_vec), (bm, "polar", polar),
                              (rp, "rodrigues_vec", rodrigues_vec), (rp, "polar", polar)):
            self._saved.append((mod, name, getattr(mod, name)))
            setattr(mod, name, fn)
        return self

    def __exit__(self, *exc):
        for mod, name, fn in reversed(self._saved):
            setattr(mod, name, fn)
        self._saved = []
        return False


# what each rig that goes round is there for: the branches it must take (tests/test_bundle_model.py, tests/test_bundle_reproj_model.py)
WIDE_TAKES = {
    "ring_8x45_center_0": ("acos mid", "acos neg", "acos pos", "quadrant 0", "quadrant 1", "quadrant 2"),
    "ring_8x45_center_4": ("acos mid", "acos neg", "acos pos", "quadrant 0", "quadrant 1", "quadrant 2"),
    "ring_8x45_exact_half_turn": ("half turn", "identity", "acos mid", "acos neg", "quadrant 2"),
    "ring_6x60_center_0": ("acos neg", "quadrant 1", "quadrant 2"),
    "arc_5x50_natural_end": ("acos mid", "acos neg", "acos pos", "quadrant 1", "quadrant 2"),
    "reflection_R_in": ("det < 0",),
    "ring_16x22p5_two_steps": ("acos mid", "acos neg", "acos pos", "quadrant 0", "quadrant 1", "quadrant 2"),
}
NARROW_NEVER = ("acos mid", "acos neg", "half turn", "det < 0")


def branches():
    """What the sweeps are there for, counted on the model's arithmetic: {branch: times taken}.  The tests assert each is positive."""
    out = {}
    q = np.array([bm._reduce(float(x))[1] for x in angles() if math.isfinite(x) and abs(x) < 1e15])
    for v in (-2, -1, 0, 1, 2):
        out["quadrant %d" % v] = int((q == v).sum())
    c = cosines()
    out.update({"acos mid": int(((c < 0.5) & (c > -0.5)).sum()), "acos neg": int((c <= -0.5).sum()), "acos pos": int((c >= 0.5).sum()),
                "acos outside": int((np.abs(c) > 1).sum())})
    th = np.sqrt((rotation_vectors() ** 2).sum(1))
    out.update({"theta below eps": int((th < bm.DBL_EPSILON).sum()), "theta above eps": int(((th >= bm.DBL_EPSILON) & (th < 1e-8)).sum())})
    small = {(below, pos): 0 for below in (True, False) for pos in (True, False)}
    flips = {True: 0, False: 0}
    for R in rotation_matrices():
        s, cc = _small_s_of(R), (((R[0] + R[4]) + R[8]) - 1.0) * 0.5
        if abs(s - 1e-5) < 1e-9 or s < 1e-5:
            small[(s < 1e-5, cc > 0)] += 1
        if s < 1e-5 and not cc > 0:
            rx, ry, rz = (math.sqrt(max((R[k] + 1.0) * 0.5, 0.0)) for k in (0, 4, 8))
            ry, rz = ry * (-1.0 if R[1] < 0 else 1.0), rz * (-1.0 if R[2] < 0 else 1.0)
            flips[abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[5] > 0) != ((ry * rz) > 0)] += 1
    out.update({"s below 1e-5, c > 0": small[(True, True)], "s below 1e-5, c <= 0": small[(True, False)], "s just above 1e-5, c > 0": small[(False, True)],
                "s just above 1e-5, c <= 0": small[(False, False)], "half turn, rz negated": flips[True], "half turn, rz kept": flips[False]})
    P = polar_inputs()
    ok = model("polar")[:, 9] == 1.0
    with np.errstate(all="ignore"):
        det = np.array([np.linalg.det(m.reshape(3, 3)) if np.isfinite(m).all() else np.nan for m in P])
    out.update({"polar det < 0": int((ok & (det < 0)).sum()), "polar det > 0": int((ok & (det > 0)).sum()), "polar not ok": int((~ok).sum())})
    return out
