#!/usr/bin/env python3
"""Generates tests/golden/ref_imgio_files.npz: the image files test_imgio.py decodes, cut from the reference's committed artefacts
without re-encoding them, so that the tests read them from the repository alone.

    python tests/golden/make_golden_imgio.py <reference tree>

  bmp/<name>  the first six .bmp files of the tree (sorted paths, as the test always took them): the file's own headers and palette,
              height cut to a band of BMP_ROWS rows from the middle of the picture (biHeight, biSizeImage and bfSize rewritten), the
              band's stored rows byte for byte.
  jpg/<name>  the first two pano.jpg files: the file's own markers and tables, the height in SOF0 cut to JPG_MCU_ROWS rows of MCUs,
              the entropy-coded segment cut after the last block of those rows (the last byte padded with 1-bits, as a scan ends).
              The coded blocks are the encoder's own; only the scan's tail is dropped.
"""
import glob
import io
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_imgio_files.npz")
BMP_ROWS = 32
JPG_MCU_ROWS = 8


def bmp_band(data, rows=BMP_ROWS):
    assert data[:2] == b"BM"
    off, = struct.unpack_from("<I", data, 10)
    width, height, _, bpp, comp = struct.unpack_from("<iiHHI", data, 18)
    assert comp == 0 and height > rows
    stride = (width * bpp // 8 + 3) // 4 * 4
    first = (abs(height) - rows) // 2
    band = data[off + first * stride: off + (first + rows) * stride]
    out = bytearray(data[:off]) + band
    struct.pack_into("<i", out, 22, rows if height > 0 else -rows)
    struct.pack_into("<I", out, 34, len(band))
    struct.pack_into("<I", out, 2, len(out))
    return bytes(out)


class _Bits:
    """MSB-first reader over an entropy-coded segment with its 0xFF00 stuffing removed; pos() is the bit position."""

    def __init__(self, data):
        self.data, self.bit = data, 0

    def read(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.data[self.bit >> 3] >> (7 - (self.bit & 7))) & 1)
            self.bit += 1
        return v


def _huff_table(counts, symbols):
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return codes


def _decode(bits, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | bits.read(1)
        if (length, code) in table:
            return table[(length, code)]
    raise ValueError("bad Huffman code")


def jpeg_band(data, mcu_rows=JPG_MCU_ROWS):
    """The baseline, non-interleaved-restart JPEG `data` cut to its first `mcu_rows` rows of MCUs."""
    assert data[:2] == b"\xff\xd8"
    i, dc, ac, comps, sof = 2, {}, {}, None, None
    while True:
        assert data[i] == 0xFF
        m, ln = data[i + 1], struct.unpack_from(">H", data, i + 2)[0]
        seg = data[i + 4:i + 2 + ln]
        if m == 0xC0:
            sof = i
            _, h, w, nc = struct.unpack_from(">BHHB", seg)
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15) for c in range(nc)]
        elif m in (0xC1, 0xC2, 0xC3, 0xDD):
            raise ValueError("only baseline JPEG without restart intervals is cut here (marker %02x)" % m)
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                tc, th = seg[j] >> 4, seg[j] & 15
                counts = seg[j + 1:j + 17]
                syms = seg[j + 17:j + 17 + sum(counts)]
                (ac if tc else dc)[th] = _huff_table(counts, syms)
                j += 17 + sum(counts)
        elif m == 0xDA:
            ns = seg[0]
            sel = {seg[1 + 2 * k]: (seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)}
            scan = i + 2 + ln
            break
        i += 2 + ln
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcux = -(-w // (8 * hmax))
    assert mcu_rows * 8 * vmax < h
    # the coded segment without its stuffing, and where each of its bytes lies in the file
    raw, where, j = bytearray(), [], scan
    while not (data[j] == 0xFF and data[j + 1] != 0x00):
        raw.append(data[j])
        where.append(j)
        j += 2 if data[j] == 0xFF else 1
    bits = _Bits(raw)
    for _ in range(mcu_rows * mcux):
        for cid, hs, vs in comps:
            td, ta = sel[cid]
            for _ in range(hs * vs):
                s = _decode(bits, dc[td])
                bits.read(s)
                k = 1
                while k < 64:
                    rs = _decode(bits, ac[ta])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    bits.read(s)
                    k += 1
    nfull, tail = bits.bit >> 3, bits.bit & 7
    out = bytearray(data[:where[nfull] if nfull < len(where) else j])
    if tail:
        last = (raw[nfull] | (0xFF >> tail)) & 0xFF
        out.append(last)
        if last == 0xFF:
            out.append(0x00)
    out += b"\xff\xd9"
    struct.pack_into(">H", out, sof + 5, mcu_rows * 8 * vmax)
    return bytes(out)


def main(ref):
    from PIL import Image
    entries = {}
    for f in sorted(glob.glob(os.path.join(ref, "**", "*.bmp"), recursive=True))[:6]:
        cut = bmp_band(open(f, "rb").read())
        im = np.asarray(Image.open(io.BytesIO(cut)).convert("RGB"))
        assert im.shape[0] == BMP_ROWS
        entries["bmp/" + os.path.relpath(f, ref)] = np.frombuffer(cut, np.uint8)
    for f in sorted(glob.glob(os.path.join(ref, "*", "*", "pano.jpg")))[:2]:
        data = open(f, "rb").read()
        cut = jpeg_band(data)
        full = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(int)
        part = np.asarray(Image.open(io.BytesIO(cut)).convert("RGB")).astype(int)
        n = part.shape[0]
        # the band decodes to the full file's rows (chroma upsampling reads one row past the band: its last rows may differ slightly)
        assert np.array_equal(part[:n - 2], full[:n - 2]) and np.abs(part - full[:n]).max() <= 32, f
        entries["jpg/" + os.path.relpath(f, ref)] = np.frombuffer(cut, np.uint8)
    np.savez_compressed(OUT, **entries)
    print("wrote", OUT, {k: v.size for k, v in entries.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
