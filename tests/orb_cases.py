"""Images for the features finder's tests (tests/test_orb_model.py, tests/test_gpu_orb*.py): seeded, small, and built so that every path
of isx_orb_find is taken - corners on several levels, empty levels, ties at both cuts.  LIMIT_CASES are the images past one pass of the
final cut, past 256 layers and at the smallest and largest sides (tests/test_orb_limit_cases.py asserts on the model what each is for)."""
import numpy as np


def scene(h, w, seed, channels=1):
    """Blobs (rectangles and discs of random gray) under seeded noise: corners of every strength, few exact ties."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 90, np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(max(6, h * w // 900)):
        cy, cx, r, v = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(3, 14)), int(rng.integers(0, 256))
        if rng.integers(0, 2):
            img[max(cy - r, 0):cy + r, max(cx - r, 0):cx + r] = v
        else:
            img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v
    img = np.clip(img + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)
    if channels == 1:
        return img
    out = np.stack([np.clip(img.astype(np.int64) + rng.integers(-20, 21, (h, w)), 0, 255).astype(np.uint8) for _ in range(channels)], axis=2)
    return np.ascontiguousarray(out)


def squares(h, w, period=16, side=6, lo=40, hi=200):
    """Bright squares on a periodic grid: the pixels around a square's corner share one FAST score, a plateau on which non-max suppression
    keeps nothing at level 0."""
    img = np.full((h, w), lo, np.uint8)
    for y in range(4, h - side, period):
        for x in range(4, w - side, period):
            img[y:y + side, x:x + side] = hi
    return img


def dots(h, w, period=8, count=None, lo=40, hi=200):
    """Lone bright pixels on a periodic grid (the first `count` of them in row-major order, all when None).  A dot is a FAST corner of
    score hi - lo - 1 whose neighbours are no corners, and every dot has the same Harris response: both cuts fall into ties."""
    img = np.full((h, w), lo, np.uint8)
    k = 0
    for y in range(36, h - 36, period):
        for x in range(36, w - 36, period):
            if count is None or k < count:
                img[y, x] = hi
            k += 1
    return img


def noise(h, w, seed):
    """Uniform noise: more FAST corners than any cut keeps, hardly a tie among the Harris responses."""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def dots_from(h, w, x0=31, y0=31, period=8, lo=40, hi=200):
    """dots() on the first pixel that can be a keypoint: lone bright pixels at (x0 + i period, y0 + j period) inside the border of 31."""
    img = np.full((h, w), lo, np.uint8)
    for y in range(y0, h - 31, period):
        for x in range(x0, w - 31, period):
            img[y, x] = hi
    return img


def flat(h, w, v=90):
    return np.full((h, w), v, np.uint8)


_STRIP = dict(nlevels=8, scale_factor=1.05, fast_threshold=5)
# name: (image, Params keywords).  One level unless said: the layer is the cell.
LIMIT_CASES = {
    # k_orb_final_cut takes 1024 candidates a pass: 2 passes, 4 passes (1920 is the largest n a level admits: 2 n + 256 = 4096)
    "passes-2": (lambda: noise(200, 200, 101), dict(grid=(1, 1), nlevels=1, n_features=1500, fast_threshold=20)),
    "passes-4": (lambda: noise(260, 260, 102), dict(grid=(1, 1), nlevels=1, n_features=1920, fast_threshold=1)),
    # every response is equal: a row is decided by the equal candidates before it, across the passes
    "passes-ties-fit": (lambda: dots(400, 400, period=6, count=1100), dict(grid=(1, 1), nlevels=1, n_features=1200)),
    "passes-ties-cut": (lambda: dots(400, 400, period=6, count=1300), dict(grid=(1, 1), nlevels=1, n_features=1200)),
    "passes-ties-full": (lambda: dots(400, 400, period=6), dict(grid=(1, 1), nlevels=1, n_features=1900)),
    # strips of 70-pixel cells, 8 levels each: 264 and 1024 layers
    "layers-264": (lambda: noise(70, 2310, 103), dict(grid=(33, 1), n_features=33 * 40, **_STRIP)),
    "layers-1024": (lambda: noise(70, 8960, 104), dict(grid=(128, 1), n_features=128 * 40, **_STRIP)),
    # the smallest sides; 62 has no interior pixel, 63 exactly one
    "side-1x1": (lambda: flat(1, 1), dict(grid=(1, 1))),
    "side-1x200": (lambda: flat(1, 200), dict(grid=(1, 1))),
    "side-200x1": (lambda: flat(200, 1), dict(grid=(1, 1))),
    "side-62x62": (lambda: flat(62, 62), dict(grid=(1, 1))),
    "side-62x62-dot": (lambda: dots_from(62, 62, 30, 30), dict(grid=(1, 1))),     # a corner one pixel outside the (empty) interior
    "side-63x63": (lambda: dots_from(63, 63), dict(grid=(1, 1))),
    "side-63x200": (lambda: dots_from(63, 200), dict(grid=(1, 1))),
    "side-3x5-cells-of-1": (lambda: noise(3, 5, 105), dict(grid=(5, 3), nlevels=4, n_features=10)),
    # ISX_ORB_MAX_SIDE: the coordinate along the long side is past 16000
    "max-side-x": (lambda: dots_from(64, 16384, x0=16384 - 200), dict(grid=(1, 1), nlevels=2, n_features=100)),
    "max-side-y": (lambda: dots_from(16384, 64, y0=16384 - 200), dict(grid=(1, 1), nlevels=2, n_features=100)),
}
SIDE_CASES = sorted(n for n in LIMIT_CASES if n.startswith("side-"))
_LIMIT_WANT = {}


def limit_want(name):
    """(image, Params, the model's Result, its stages, the model's seconds) of a limit case: computed once a process, shared by every
    test module that asks, and never written to"""
    if name not in _LIMIT_WANT:
        import time
        from helpers import orb_np
        make, kw = LIMIT_CASES[name]
        img, p, stages = make(), orb_np.Params(**kw), {}
        t0 = time.perf_counter()
        want = orb_np.find(img, p, stages=stages)
        _LIMIT_WANT[name] = (img, p, want, stages, time.perf_counter() - t0)
    return _LIMIT_WANT[name]
