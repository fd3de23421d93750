#!/usr/bin/env python3
"""Records tests/golden/bundle_reproj_chain64.npz: the model's outputs (tests/helpers/bundle_reproj_np.py) on the chain of 64 images of
tests/bundle_reproj_cases.py (448 unknowns, max_iter 1), the largest system the entry takes, which the suite does not solve in Python in
every run.  The inputs are regenerated from their seed by the test; cameras_in and the first keypoints are stored to show that they are the
same ones.

    python tests/golden/make_golden_bundle_reproj.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bundle_reproj_cases as cases  # noqa: E402
from helpers import bundle_reproj_np as rp  # noqa: E402


def main():
    c = cases.chain_64()
    cams, kr, rs, re = rp.adjust(c["sizes"], c["keypoints"], c["pairs"], c["matches"], c["masks"], c["counts"], c["conf"], c["est_rig_stats"],
                                 c["cameras_in"], c["rig_first"], c["conf_thresh"], c["max_iter"], refine_flags=c["refine_flags"])
    out = dict(cameras=cams, kr32=kr, rig_stats=rs, rig_err=re, cameras_in=c["cameras_in"], max_iter=np.int32(c["max_iter"]))
    for i in range(3):
        out["keypoints_%d" % i] = c["keypoints"][i]
    path = os.path.join(HERE, "bundle_reproj_chain64.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; rig_stats", rs.tolist(), "rig_err", re.tolist())


if __name__ == "__main__":
    main()
