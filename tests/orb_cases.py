"""Images for the features finder's tests (tests/test_orb_model.py, tests/test_gpu_orb*.py): seeded, small, and built so that every path
of isx_orb_find is taken - corners on several levels, empty levels, ties at both cuts."""
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
