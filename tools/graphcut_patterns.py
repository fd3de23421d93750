"""The structured image patterns of the graph-cut tests and of the fuzz family case_graphcut_grad (tools/fuzz_parity.py): constants, ramps, a
step, a checkerboard and one-pixel serpentines, two images a pattern.  NumPy only.  tests/graphcut_cases.py builds its tiles, corners and
masks on these; the fuzz tool draws a pattern at random sizes.  Kept beside the tool so that the tool needs nothing of the tests but their
models."""
import numpy as np

PATTERNS = ("identical", "const_10_13", "const_0_255", "ramp_rev", "xramp_yramp", "step_inv", "checker_inv", "serp_0", "serp_serp", "channels")


def serpentine(h, w):
    """One-pixel serpentine: rows 1, 5, 9, ... are 255, joined alternately at the last and the first column over the next three rows."""
    a = np.zeros((h, w), np.uint8)
    for k, r in enumerate(range(1, h, 4)):
        a[r] = 255
        a[r + 1:r + 4, w - 1 if k % 2 == 0 else 0] = 255
    return a


def pattern_images(name, h, w):
    """The two h x w x 3 uint8 images of a pattern."""
    yy, xx = np.mgrid[0:h, 0:w]
    xramp = xx * 255 // max(w - 1, 1)
    yramp = yy * 255 // max(h - 1, 1)
    step = np.where(xx >= 2 * w // 3, 255, 0)
    if name == "identical":
        pair = (np.full((h, w), 50), np.full((h, w), 50))
    elif name == "const_10_13":
        pair = (np.full((h, w), 10), np.full((h, w), 13))
    elif name == "const_0_255":
        pair = (np.full((h, w), 0), np.full((h, w), 255))
    elif name == "ramp_rev":
        pair = (xramp, xramp[:, ::-1])
    elif name == "xramp_yramp":
        pair = (xramp, yramp)
    elif name in ("step_inv", "channels"):
        pair = (step, 255 - step)
    elif name == "checker_inv":
        c = ((xx + yy) & 1) * 255
        pair = (c, 255 - c)
    elif name == "serp_0":
        pair = (serpentine(h, w), np.zeros((h, w)))
    elif name == "serp_serp":
        s = serpentine(h, w)
        pair = (s, s[::-1])
    else:
        raise KeyError(name)
    imgs = []
    for a in pair:
        img = np.zeros((h, w, 3), np.uint8)
        if name == "channels":
            img[:, :, 1] = a                                      # channel 1 only: the one pattern without equal channels
        else:
            img[:, :, :] = np.asarray(a)[:, :, None]
        imgs.append(img)
    return imgs
