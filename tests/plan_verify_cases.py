"""The fixed cameras of the planned-ROI verification tests (tests/test_plan_verify_model.py on the CPU, tests/test_gpu_plan_verify.py on the
GPU), one named class each.  The verifier reads the projection and the source SIZE, never an image, so every source is small; the sizes
sit on the scans' launch geometry: 256 x 128 and 257 x 129 (one and two k_roi_scan blocks each way: 256 columns, ROI_ROWS = 128 rows a
block), 33 x 33, and 700 x 500, whose 2 (W + H) = 2400 border pixels take three passes of the border scan's 1024 threads and whose full scan
is 3 x 4 blocks.  Scales run from 0.5 f to 2 f.

A case: (class, kind, src_w, src_h, f, cx, cy, scale, yaw, pitch, roll), K = [[f, 0, cx], [0, f, cy], [0, 0, 1]], R = Ry(yaw) Rx(pitch) Rz(roll).

Classes (CLASSES; what each must be is checked by tests/test_plan_verify_model.py::test_every_case_is_of_its_class):
    cyl_light          cylindrical, extrema provably on the border: the one-workgroup scan `roi_border` (verify_is_light = 1)
    cyl_corner_behind  cylindrical, a corner with z_ <= 1e-6: full scan `roi_scan`
    cyl_pole           cylindrical, the cylinder's pole within 2 px outside the image: full scan
    cyl_pole_inside    cylindrical, the pole inside the image (some corner is then behind the camera as well): full scan
    cyl_rolled         cylindrical, R[1][1] <= 0 by a roll past 90 degrees: full scan
    sph_plain          spherical, no pole inside: `roi_border_sph`
    sph_north          spherical, the north pole (v = pi scale) inside the image
    sph_south          spherical, the south pole (v = 0) inside the image
    cyl_straddle       cylindrical, the tile straddles u = +-pi scale (the camera looks backwards)
    sph_straddle       spherical, the same
    cyl_on_seam        cylindrical, a pixel exactly on the back seam: br.u = (int)(scale pi_f), the largest value a u bound can take
    sph_on_seam        spherical, the same
    sph_north_edge     spherical, the north pole inside the image within a pixel of its border: the border's largest v truncates to
                       (int)(pi scale) - 1, which a plan must not be allowed to carry
    sph_south_edge     spherical, the south pole inside the image within a pixel of its border: the border's smallest v truncates to 1
    sph_pole_one_sided spherical, a pole inside the image whose border stays on one side of u = 0 by a pixel or more: tl.u = 0 is the pole's
    zero_bound         a bound that truncates to 0 (R = I, the principal point at a fraction of a pixel: from below and from above)
    all_negative       all four bounds negative
    all_positive       all four bounds positive
"""
import numpy as np

CYL, SPH = 0, 1
PI = float(np.pi)

CASES = [
    # ---- cylindrical, light
    ("cyl_light", CYL, 129, 46, 247.8, 67.2, 21.9, 178.4, -0.092, 0.262, -0.036),
    ("cyl_light", CYL, 179, 150, 229.0, 91.0, 75.2, 123.7, -0.204, 0.231, -0.079),
    ("cyl_light", CYL, 256, 128, 157.3, 126.2, 62.6, 173.0, 0.3, -0.176, -0.006),
    ("cyl_light", CYL, 129, 46, 254.0, 65.8, 23.2, 492.8, -0.268, -0.271, 0.188),
    ("cyl_light", CYL, 33, 33, 55.7, 14.4, 16.4, 108.6, 0.474, -0.062, 0.036),
    ("cyl_light", CYL, 48, 64, 94.6, 26.0, 34.3, 177.8, 0.192, -0.204, 0.107),
    ("cyl_light", CYL, 700, 500, 329.2, 350.1, 249.8, 181.1, 0.501, 0.103, 0.006),
    ("cyl_light", CYL, 257, 129, 204.6, 126.7, 65.7, 106.4, -0.359, -0.104, -0.199),
    ("cyl_light", CYL, 257, 129, 115.3, 131.3, 65.4, 78.4, -0.086, 0.019, 0.149),
    # ---- cylindrical, outside the proof
    ("cyl_corner_behind", CYL, 129, 46, 40.1, 67.2, 21.9, 28.9, 1.23, 0.262, -0.036),
    ("cyl_corner_behind", CYL, 100, 75, 40.5, 51.7, 36.3, 40.1, 1.022, -0.293, -0.039),
    ("cyl_corner_behind", CYL, 256, 128, 176.1, 130.9, 66.8, 216.6, 0.996, 0.033, -0.089),
    ("cyl_corner_behind", CYL, 256, 128, 178.1, 127.7, 64.0, 156.7, -1.273, 0.396, 0.117),
    ("cyl_corner_behind", CYL, 179, 150, 122.7, 90.8, 77.0, 180.4, -1.383, -0.228, 0.056),
    ("cyl_corner_behind", CYL, 700, 500, 241.8, 351.8, 250.5, 207.9, 0.996, -0.053, -0.008),
    ("cyl_pole", CYL, 64, 48, 42.1, 32.0, 21.5, 81.3, -0.003, 1.062, -0.039),
    ("cyl_pole", CYL, 64, 48, 46.4, 31.6, 23.7, 53.8, 0.104, -1.06, -0.155),
    ("cyl_pole", CYL, 33, 33, 25.4, 15.6, 18.1, 16.5, -0.036, -1.014, -0.061),
    ("cyl_pole", CYL, 33, 33, 23.8, 14.4, 13.8, 13.6, 0.069, 1.003, 0.005),
    ("cyl_pole", CYL, 33, 33, 26.1, 18.8, 14.5, 35.5, -0.137, 1.025, -0.136),
    ("cyl_pole_inside", CYL, 33, 33, 20.0, 16.5, 16.5, 24.0, 0.1, -1.5, 0.05),
    ("cyl_rolled", CYL, 48, 64, 52.5, 22.7, 31.9, 85.6, 0.577, 0.369, -2.272),
    ("cyl_rolled", CYL, 129, 46, 160.7, 61.9, 23.8, 191.2, 0.423, 0.074, -2.616),
    ("cyl_rolled", CYL, 33, 33, 57.3, 14.8, 17.3, 52.7, 0.366, 0.371, 2.205),
    ("cyl_rolled", CYL, 256, 128, 370.2, 130.2, 64.8, 425.7, 0.372, -0.127, 1.876),
    ("cyl_rolled", CYL, 257, 129, 227.4, 127.0, 64.2, 209.2, 0.005, 0.043, -2.562),
    # ---- spherical
    ("sph_plain", SPH, 129, 46, 247.8, 67.2, 21.9, 178.4, -0.092, 0.262, -0.036),
    ("sph_plain", SPH, 256, 128, 157.3, 126.2, 62.6, 173.0, 0.3, -0.176, -0.006),
    ("sph_plain", SPH, 33, 33, 55.7, 14.4, 16.4, 108.6, 0.474, -0.062, 0.036),
    ("sph_plain", SPH, 700, 500, 329.2, 350.1, 249.8, 181.1, 0.501, 0.103, 0.006),
    ("sph_plain", SPH, 257, 129, 204.6, 126.7, 65.7, 106.4, -0.359, -0.104, -0.199),
    ("sph_north", SPH, 129, 46, 247.8, 67.2, 21.9, 178.4, -0.092, -1.541, -0.036),
    ("sph_north", SPH, 129, 46, 93.6, 66.0, 21.7, 83.3, -0.018, -1.436, 0.185),
    ("sph_north", SPH, 33, 33, 61.6, 16.7, 16.3, 34.5, -0.525, -1.515, 0.141),
    ("sph_north", SPH, 64, 48, 38.3, 30.1, 23.4, 61.3, -0.322, -1.286, -0.044),
    ("sph_north", SPH, 700, 500, 695.2, 350.1, 251.5, 417.1, -0.371, -1.422, 0.014),
    ("sph_north", SPH, 257, 129, 501.6, 128.5, 64.5, 406.3, 0.498, -1.511, -0.074),
    ("sph_north", SPH, 256, 128, 293.5, 128.0, 63.0, 478.4, 0.392, -1.4, 0.138),
    ("sph_south", SPH, 129, 46, 247.8, 67.2, 21.9, 178.4, -0.092, 1.601, -0.036),
    ("sph_south", SPH, 33, 33, 61.6, 16.7, 16.3, 34.5, -0.525, 1.627, 0.141),
    ("sph_south", SPH, 100, 75, 194.2, 49.9, 39.9, 141.8, -0.093, 1.675, -0.19),
    ("sph_south", SPH, 64, 48, 38.3, 30.1, 23.4, 61.3, -0.322, 1.856, -0.044),
    ("sph_south", SPH, 256, 128, 359.7, 126.1, 61.4, 521.6, -0.106, 1.709, 0.126),
    ("sph_south", SPH, 257, 129, 357.9, 129.6, 65.4, 619.2, -0.113, 1.717, -0.042),
    # ---- the back seam u = +-pi scale
    ("cyl_straddle", CYL, 100, 75, 83.8, 50.9, 38.8, 42.7, 3.225, -0.174, -0.114),
    ("cyl_straddle", CYL, 64, 48, 38.3, 30.1, 23.4, 61.3, 3.426, 0.273, -0.044),
    ("cyl_straddle", CYL, 33, 33, 30.5, 15.4, 17.7, 48.2, 3.086, 0.31, 0.093),
    ("cyl_straddle", CYL, 257, 129, 118.8, 128.5, 62.3, 72.5, 3.189, 0.071, 0.003),
    ("cyl_straddle", CYL, 257, 129, 218.4, 130.6, 64.1, 303.6, 3.206, 0.006, 0.005),
    ("sph_straddle", SPH, 129, 46, 247.8, 67.2, 21.9, 178.4, 3.171, 0.262, -0.036),
    ("sph_straddle", SPH, 129, 46, 93.6, 66.0, 21.7, 83.3, 3.276, 0.385, 0.185),
    ("sph_straddle", SPH, 33, 33, 61.6, 16.7, 16.3, 34.5, 3.197, 0.113, 0.141),
    ("sph_straddle", SPH, 256, 128, 184.6, 125.0, 66.0, 193.8, 3.147, -0.186, 0.152),
    # ---- a pixel exactly on the back seam (yaw = pi, no roll, cx an integer): the extremum IS +-scale pi_f
    ("cyl_on_seam", CYL, 179, 150, 100.0, 89.0, 75.3, 70.8, PI, 0.1, 0.0),
    ("cyl_on_seam", CYL, 64, 48, 50.0, 31.0, 24.2, 77.7, PI, -0.2, 0.0),
    ("sph_on_seam", SPH, 179, 150, 100.0, 89.0, 75.3, 70.8, PI, 0.1, 0.0),
    ("sph_on_seam", SPH, 64, 48, 50.0, 31.0, 24.2, 77.7, PI, -0.2, 0.0),
    # ---- a pole of the sphere inside the image less than a pixel from its border: the border's extremum lies in the pole's own pixel or the next
    ("sph_north_edge", SPH, 129, 46, 124.2, 64.3, 22.6, 73.6, 0.2, -1.38885, 0.0),
    ("sph_north_edge", SPH, 33, 33, 40.0, 16.4, 16.0, 30.0, 1.0, -1.1817, 0.0),
    ("sph_north_edge", SPH, 257, 129, 300.0, 128.3, 64.0, 250.0, 0.1, -1.36205, 0.0),
    ("sph_south_edge", SPH, 129, 46, 60.0, 64.4, 22.6, 118.0, 0.2, 1.92151, 0.0),
    ("sph_south_edge", SPH, 33, 33, 30.0, 16.45, 16.0, 58.0, 1.0, 2.04505, 0.0),
    ("sph_south_edge", SPH, 257, 129, 150.0, 128.5, 64.0, 290.0, 0.1, 1.97012, 0.0),
    # ---- the south pole inside the image, beside the first row, and a border that does not wind around it: all its u on one side of 0
    ("sph_pole_one_sided", SPH, 100, 75, 121.1, 51.9, 38.2, 82.8, -1.58272, 1.87053, 0.0),
    # ---- signs of the bounds
    ("zero_bound", SPH, 100, 75, 92.8, 0.3, 0.0, 155.9, 0.0, 0.0, 0.0),
    ("zero_bound", CYL, 100, 75, 150.6, 49.4, 0.3, 116.0, 0.0, 0.0, 0.0),
    ("zero_bound", CYL, 33, 33, 26.8, 0.1, 14.3, 44.0, 0.0, 0.0, 0.0),
    ("zero_bound", CYL, 64, 48, 65.8, 34.0, -0.1, 55.9, 0.0, 0.0, 0.0),
    ("zero_bound", SPH, 33, 33, 54.1, 0.5, 0.0, 69.8, 0.0, 0.0, 0.0),
    ("all_negative", CYL, 179, 150, 211.5, 87.3, 75.0, 173.4, -0.91, 0.56, 0.108),
    ("all_negative", CYL, 48, 64, 75.0, 23.5, 32.5, 138.0, -1.031, 0.854, 0.168),
    ("all_negative", CYL, 256, 128, 250.0, 128.6, 62.6, 160.0, -0.996, 0.76, -0.161),
    ("all_positive", SPH, 100, 75, 126.1, 51.7, 36.3, 124.8, 0.781, -0.605, -0.039),
    ("all_positive", CYL, 64, 48, 84.7, 33.6, 25.7, 166.0, 0.976, -0.7, 0.167),
    ("all_positive", SPH, 257, 129, 362.0, 130.1, 61.7, 376.5, 0.751, -0.589, -0.009),
]

CLASSES = ["cyl_light", "cyl_corner_behind", "cyl_pole", "cyl_pole_inside", "cyl_rolled", "sph_plain", "sph_north", "sph_south", "cyl_straddle",
           "sph_straddle", "cyl_on_seam", "sph_on_seam", "sph_north_edge", "sph_south_edge", "sph_pole_one_sided",
           "zero_bound", "all_negative", "all_positive"]
REQUIRED_SIZES = [(256, 128), (257, 129), (33, 33), (700, 500)]
NO_CLAIM_CAP = 0.10        # of the shifted plans over the whole list


def rotation(yaw, pitch, roll):
    a, b, c = pitch, yaw, roll
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return (Ry @ Rx @ Rz).astype(np.float32)


def camera(case):
    """-> (kind, scale, K, R, src_w, src_h)"""
    _cls, kind, w, h, f, cx, cy, scale, yaw, pitch, roll = case
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float32)
    return kind, float(np.float32(scale)), K, rotation(yaw, pitch, roll), w, h


def case_id(case):
    return "%s-%s-%dx%d-s%g" % (case[0], "cyl" if case[1] == CYL else "sph", case[2], case[3], case[7])


_TRUTH = {}


def truth(oracle, i):
    """The oracle's extrema and ROI of case i and the model's verdict on its true plan and its eight shifts: computed once, shared, read-only."""
    from helpers import plan_verify_np as M
    if i not in _TRUTH:
        kind, scale, K, R, w, h = camera(CASES[i])
        t = M.truth(oracle, kind, scale, K, R, w, h)
        t["scan"] = M.scan_kind(kind, K, R, t["r_kinv"], w, h)
        t["plans"] = [(None, list(t["roi"]))] + [((k, s), M.shifted(t["roi"], k, s)) for k, s in M.SHIFTS]
        t["verdicts"] = [M.verdict(kind, scale, p, t["extrema"], t["north"], t["south"]) for _sh, p in t["plans"]]
        _TRUTH[i] = t
    return _TRUTH[i]
