"""Writes tests/golden/ref_orb_artifact.npz from the two images the reference's features demo commits (F = its 特征点检测 demo):

    gray    the gray of src1.bmp, (B*1868 + G*9617 + R*4899 + 8192) >> 14, uint8
    drawn   np.packbits of the pixels where 重构的特征点.bmp differs from src1.bmp in any channel: what drawKeypoints of F's restated finder put
            on top of src1.bmp (a radius-3 circle per keypoint)
    shape   (rows, cols)

Data the reference's program wrote, no program text.  Run where the reference tree is (python tests/golden/make_golden_orb.py <reference
root>); never on a GPU box, nothing at test time reads the reference.  When the whole image passes the repository's 1 MiB limit, cell 0
of the 3 x 1 grid is written instead (cols // 3 columns)."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 1 << 20


def read_bmp(path):
    """an uncompressed 24- or 32-bit BMP as (rows, cols, 3) uint8 BGR"""
    raw = open(path, "rb").read()
    assert raw[:2] == b"BM", path
    offset = struct.unpack_from("<I", raw, 10)[0]
    w, h = struct.unpack_from("<ii", raw, 18)
    planes, bpp, compression = struct.unpack_from("<HHI", raw, 26)
    assert planes == 1 and bpp in (24, 32) and compression == 0, (path, bpp, compression)
    pitch = (w * (bpp // 8) + 3) & ~3
    rows = np.frombuffer(raw, np.uint8, pitch * abs(h), offset).reshape(abs(h), pitch)[:, :w * (bpp // 8)].reshape(abs(h), w, bpp // 8)
    if h > 0:
        rows = rows[::-1]
    return np.ascontiguousarray(rows[:, :, :3])


def main(root):
    d = os.path.join(root, "特征点检测", "特征点检测")
    src = read_bmp(os.path.join(d, "src1.bmp"))
    marked = read_bmp(os.path.join(d, "重构的特征点.bmp"))
    assert src.shape == marked.shape
    b, g, r = (src[:, :, i].astype(np.int64) for i in range(3))
    gray = ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)
    drawn = (src != marked).any(axis=2)
    out = os.path.join(HERE, "ref_orb_artifact.npz")
    for cols in (gray.shape[1], gray.shape[1] // 3):
        gy, dr = np.ascontiguousarray(gray[:, :cols]), np.ascontiguousarray(drawn[:, :cols])
        np.savez_compressed(out, gray=gy, drawn=np.packbits(dr), shape=np.array(gy.shape, np.int64), whole=np.array(cols == gray.shape[1]))
        if os.path.getsize(out) < LIMIT:
            break
    print(out, os.path.getsize(out), "bytes;", gy.shape, "pixels,", int(dr.sum()), "drawn of", int(drawn.sum()))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_orb.py <root of the reference tree>")
    main(sys.argv[1])
