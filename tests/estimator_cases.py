"""The named cases of tests/test_gpu_estimator.py and the building blocks of tools/fuzz_estimator.py: synthetic inputs of
isx_estimate_cameras.  No RANSAC run: a homography is H_ij = K R_j^T R_i K^-1 / h22 for planted rotations and one focal (points are centred,
so K = diag(f, f, 1)), or a seeded well-conditioned matrix.  A case is a dict: sizes ((width, height) per image), pairs ((from, to), from <
to, global indices), H (num_pairs x 3 x 3 float64), stats (num_pairs x 8 int32: column 0 the status bits, column 1 num_inliers), rig_first
(None or the image offsets), focals_in (None or n x 4)."""
import itertools

import numpy as np

ST_H = 1


def rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def planted_rotations(n, rng):
    """Yaw, pitch and roll of every camera with magnitude in [0.1, 0.3] and a random sign."""
    ang = rng.uniform(0.1, 0.3, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    return [rotation(*a) for a in ang]


def homography(Ri, Rj, focal):
    """The homography of the pair (i, j) between centred image coordinates, normalised to h22 = 1."""
    K = np.diag([focal, focal, 1.0])
    H = K @ Rj.T @ Ri @ np.linalg.inv(K)
    return H / H[2, 2]


def all_pairs(n, first=0):
    return [(first + i, first + j) for i, j in itertools.combinations(range(n), 2)]


def make(n, pairs, seed, focal=900.0, weights=None, no_h=(), sizes=None, generic=False):
    """One rig of n images.  weights: None (seeded, 20 .. 400), an int (all equal) or a list; no_h: the pairs (by position) whose status
    bit is clear; generic: seeded matrices I + uniform(-0.2, 0.2) with H[2, :2] scaled to 1e-4 in place of the planted rotations."""
    rng = np.random.default_rng(seed)
    Rs = planted_rotations(n, rng)
    H = np.zeros((len(pairs), 3, 3))
    for k, (i, j) in enumerate(pairs):
        if generic:
            m = np.eye(3) + rng.uniform(-0.2, 0.2, (3, 3))
            m[2, :2] *= 1e-4
            m[:2, 2] *= 100.0
            H[k] = m / m[2, 2]
        else:
            H[k] = homography(Rs[i], Rs[j], focal)
    stats = np.zeros((len(pairs), 8), np.int32)
    stats[:, 0] = ST_H
    if weights is None:
        stats[:, 1] = rng.integers(20, 400, len(pairs))
    else:
        stats[:, 1] = weights
    for k in no_h:
        stats[k, 0], stats[k, 1] = 0, 0
        H[k] = 0.0
    if sizes is None:
        sizes = [(int(rng.integers(300, 2000)), int(rng.integers(200, 1500))) for _ in range(n)]
    return dict(sizes=list(sizes), pairs=list(pairs), H=H, stats=stats, rig_first=None, focals_in=None, rotations=Rs, focal=focal)


def join(rigs):
    """Several one-rig cases as the rigs of one call."""
    sizes, pairs, Hs, sts, first, fin = [], [], [], [], [0], []
    for r in rigs:
        a = first[-1]
        sizes += r["sizes"]
        pairs += [(i + a, j + a) for i, j in r["pairs"]]
        Hs.append(r["H"])
        sts.append(r["stats"])
        first.append(a + len(r["sizes"]))
        fin.append(r["focals_in"])
    assert all(f is None for f in fin) or all(f is not None for f in fin)
    return dict(sizes=sizes, pairs=pairs, H=np.concatenate(Hs), stats=np.concatenate(sts), rig_first=first,
                focals_in=None if fin[0] is None else np.concatenate(fin))


def pure_yaw_chain(n):
    """A chain whose every H is a pure yaw: h[6] * h[7] = 0 and h[0] * h[1] + h[3] * h[4] = 0, so both focals are "not ok" (-0 / 0)."""
    pairs = [(i, i + 1) for i in range(n - 1)]
    c = make(n, pairs, 11)
    for k in range(len(pairs)):
        c["H"][k] = homography(rotation(0.0, 0.0, 0.0), rotation(0.1 + 0.02 * k, 0.0, 0.0), 700.0)
    return c


def named():
    out = {}
    out["demo_2_images_1_pair"] = make(2, [(0, 1)], 1)
    out["chain_3"] = make(3, [(0, 1), (1, 2)], 2)
    out["complete_5"] = make(5, all_pairs(5), 3)
    out["complete_7"] = make(7, all_pairs(7), 4)
    out["complete_9"] = make(9, all_pairs(9), 5)
    out["complete_17"] = make(17, all_pairs(17), 6)
    out["complete_64"] = make(64, all_pairs(64), 7)
    out["all_weights_equal"] = make(6, all_pairs(6), 8, weights=50)
    p8 = all_pairs(8)
    out["two_components_5_3"] = make(8, p8, 9, no_h=[k for k, (i, j) in enumerate(p8) if (i < 5) != (j < 5)])
    out["two_components_4_4"] = make(8, p8, 10, no_h=[k for k, (i, j) in enumerate(p8) if (i < 4) != (j < 4)])
    out["fallback_focal"] = pure_yaw_chain(5)
    c = make(4, all_pairs(4), 12)
    c["focals_in"] = np.array([[880.0, 1.0, 512.0, 384.0], [910.5, 1.01, 500.25, 390.0], [899.0, 0.99, 640.0, 360.0], [905.0, 1.0, 333.0, 222.0]])
    out["focals_given"] = c
    c = make(4, all_pairs(4), 13, generic=True, weights=[400, 300, 10, 10, 350, 10])
    c["H"][0] = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 1.0]])            # determinant exactly 0: the dual is nine zeros
    c["H"][1] = np.diag([1e-160, 1e-160, 1.0])                                            # a denormal determinant: 1 / d is inf, 0 * inf NaN
    out["singular_H"] = c
    return out
