"""Device mats at the library's addressing limits, inside a guard band - the large-pitch siblings of tests/helpers/guarded.py.

The hot kernels address a mat with 32-bit byte offsets built from 24-bit multiplies (__umul24(y, step) + x * px); the host chooses between
them, a generic size_t kernel and ISX_ERR_UNSUPPORTED by  step < 2^24,  step * rows < 2^31 (sources)  and  step * rows < 2^32
(destinations).  The layouts here put a small view (24-70 columns) on either side of each of these:

    "wide"        pitch 2^24 (the default) or 2^24 + 64: the first pitch a 24-bit multiply truncates
    "wide_below"  pitch 2^24 - 64 (2^24 - 4 for a one-byte, one-channel mat): the fast side of that edge
    "tall31"      pitch 2^23: 255 rows give step * rows < 2^31, 256 rows exactly 2^31
                  (or pitch 2^24: 129 rows end past 2^31 - a source the size_t kernels serve whole)
    "tall32"      pitch 2^23 (the default; 511 / 512 rows) or 2^24 - 64 (256 / 257 rows): either side of step * rows = 2^32

    g = wide_guarded((h, w, 3), np.uint8, "tall31", seed)        # the interface of guarded.Guarded: .view .set() .get() .check()

Placement - why a wrong offset is a finding and never a fault.  A kernel that takes the fast path past its limit computes, for a byte
that belongs at offset o = y * step + x from the view's first byte, one of
    (y * (step mod 2^24)) + x          the step truncated to 24 bits:  0 <= wrong <= o
    o mod 2^32                         the sum wrapped at 32 bits:     0 <= wrong <= o
    o - 2^32  for o >= 2^31            the sum read as a signed int:   -2^31 <= wrong < 0
    o         with rows past 2^32      (a destination the host let through): the right address, inside the view
or a combination of them, which stays inside [-2^31, max(span, 2^32)), span = (rows - 1) * step + row bytes.  So the view's first byte
lies behind a lead of 2^31 + 64 KiB for the tall layouts (the wide ones span less than 2^31 bytes - no offset of theirs has the sign bit - and get 64 KiB), and the allocation
runs on to at least 2^32 + 64 KiB past the view's first byte for "tall32" and at least 64 KiB past the view's last byte for every
layout: each of the wrong addresses above lies inside this one allocation, where check() finds the byte that changed.

The buffer is torch.empty, filled on the device from a seeded torch.Generator in chunks of 256 MiB.  check() draws the same chunks again
from the same seed and compares chunk by chunk: no second copy of the buffer exists, only the view's own bytes (a few KB) are
snapshotted.  `written=` / NOTHING and GuardError.region mean what they mean in guarded.py: above / below = before the view's first /
after its last byte, lead = the 64 bytes before a row, pad = the rest of the gap between two rows, view = inside it.
"""
import collections

import numpy as np

from .guarded import NOTHING, GuardError

LAYOUTS = ("wide", "wide_below", "tall31", "tall32")
CHUNK = 256 << 20
KIB64 = 64 << 10
_PITCHES = {"wide": (1 << 24, (1 << 24) + 64), "wide_below": ((1 << 24) - 64,), "tall31": (1 << 23, 1 << 24), "tall32": (1 << 23, (1 << 24) - 64)}

Plan = collections.namedtuple("Plan", "pitch rows row_bytes offset span nbytes")


def plan(shape, dtype, layout, pitch=None):
    """The layout arithmetic alone (no torch): pitch, rows, bytes per row, the offset of the view's first byte from the 256-byte aligned
    start of the buffer, the view's span (first to last byte) and the buffer's size."""
    assert layout in LAYOUTS and len(shape) in (2, 3), (layout, shape)
    h, w = int(shape[0]), int(shape[1])
    cn = int(shape[2]) if len(shape) == 3 else 1
    es = np.dtype(dtype).itemsize
    if pitch is None:
        pitch = (1 << 24) - 4 if (layout == "wide_below" and es * cn == 1) else _PITCHES[layout][0]
    assert pitch in _PITCHES[layout] or (layout == "wide_below" and es * cn == 1 and pitch == (1 << 24) - 4), (layout, pitch)
    row_bytes = w * cn * es
    assert h >= 1 and 0 < row_bytes <= pitch - 64 and pitch % es == 0
    offset = ((1 << 31) if layout.startswith("tall") else 0) + KIB64         # a multiple of 256: every element type is aligned
    span = (h - 1) * pitch + row_bytes
    end = offset + span + KIB64
    if layout == "tall32":
        end = max(end, offset + (1 << 32) + KIB64)
    return Plan(pitch, h, row_bytes, offset, span, end)


def bytes_needed(shape, dtype, layout, pitch=None):
    """Device memory a mat of this layout takes while it is checked: the buffer and two chunks (the regenerated fill, the comparison)."""
    return plan(shape, dtype, layout, pitch).nbytes + 256 + 2 * CHUNK


class WideGuarded:
    where = "device"

    def __init__(self, shape, dtype, layout, seed, name=None, pitch=None):
        import torch
        self.shape = tuple(int(v) for v in shape)
        self.dtype = np.dtype(dtype)
        self.layout, self.name, self.seed = layout, name, int(seed)
        p = plan(self.shape, self.dtype, layout, pitch)
        self.pitch, self.row_bytes, self.offset, self.nbytes = p.pitch, p.row_bytes, p.offset, p.nbytes
        h = self.shape[0]
        cn = self.shape[2] if len(self.shape) == 3 else 1
        es = self.dtype.itemsize
        raw = torch.empty(self.nbytes + 256, dtype=torch.uint8, device="cuda")
        base = (-raw.data_ptr()) % 256
        self._raw = raw
        self.buf = raw[base:base + self.nbytes]
        gen = self._generator()
        for c0 in range(0, self.nbytes, CHUNK):
            self.buf[c0:min(c0 + CHUNK, self.nbytes)].random_(0, 256, generator=gen)
        flat = self.buf[self.offset:self.offset + p.span].view(getattr(torch, self.dtype.name))
        strides = (self.pitch // es, cn, 1) if len(self.shape) == 3 else (self.pitch // es, 1)
        self.view = flat.as_strided(self.shape, strides)
        self._bytes = self.buf[self.offset:self.offset + p.span].as_strided((h, self.row_bytes), (self.pitch, 1))     # the view's bytes
        assert self.view.data_ptr() == self.buf.data_ptr() + self.offset and self.view.data_ptr() % 256 == 0
        self.snapshot()

    def _generator(self):
        import torch
        return torch.Generator(device="cuda").manual_seed(self.seed)

    # ---- content (as guarded.Guarded) ----------------------------------------------------------------------------------------------------
    def snapshot(self):
        """Remember the view's bytes as they are now (everything else is the seeded fill); check() compares with this."""
        self._snap = self._bytes.clone()
        return self

    def set(self, array):
        import torch
        a = np.ascontiguousarray(np.asarray(array), self.dtype).reshape(self.shape)
        self.view.copy_(torch.from_numpy(a))
        return self.snapshot()

    def get(self):
        return self.view.cpu().numpy()

    # ---- the check ------------------------------------------------------------------------------------------------------------------------
    def _may_change(self, written):
        """Boolean (h, row_bytes): True where the call may write."""
        h, w = self.shape[:2]
        px = self.row_bytes // w
        if written is None:
            m = np.ones((h, w), bool)
        elif isinstance(written, str) or written is False:
            assert written in (NOTHING, False)
            m = np.zeros((h, w), bool)
        elif isinstance(written, tuple) and len(written) == 2 and not isinstance(written[0], (tuple, list, np.ndarray)):
            m = np.zeros((h, w), bool)
            m[:, max(0, int(written[0])):max(0, min(w, int(written[1])))] = True
        else:
            m = np.asarray(written, bool)
            assert m.shape == (h, w), (m.shape, (h, w))
        return np.repeat(m, px, axis=1)

    def _region(self, i):
        rel = i - self.offset
        if rel < 0:
            return "above", -1, i
        row, col = divmod(rel, self.pitch)
        if row >= self.shape[0] or (row == self.shape[0] - 1 and col >= self.row_bytes):
            return "below", row, col
        if col < self.row_bytes:
            return "view", row, col
        return ("lead" if col >= self.pitch - 64 else "pad"), row, col

    def check(self, written=None):
        """Raises GuardError when a byte of the buffer outside `written` differs from the seeded fill (inside the view: from the snapshot).
        written: None = the whole view may have changed; (c0, c1) = its columns [c0, c1); a boolean (h, w) array; NOTHING = no byte."""
        import torch
        free = torch.from_numpy(self._may_change(written)).to(self.buf.device)
        expect = torch.where(free, self._bytes, self._snap)                     # (h, row_bytes): what the view's bytes must be now
        gen = self._generator()
        scratch = torch.empty(min(CHUNK, self.nbytes), dtype=torch.uint8, device=self.buf.device)
        count, first = 0, None
        for c0 in range(0, self.nbytes, CHUNK):
            c1 = min(c0 + CHUNK, self.nbytes)
            exp = scratch[:c1 - c0].random_(0, 256, generator=gen)
            r0 = max(0, (c0 - self.offset - self.row_bytes) // self.pitch)
            for r in range(r0, self.shape[0]):
                a = self.offset + r * self.pitch                                # this row's bytes are buffer bytes [a, b)
                b = a + self.row_bytes
                if a >= c1:
                    break
                lo, hi = max(a, c0), min(b, c1)
                if lo < hi:
                    exp[lo - c0:hi - c0] = expect[r, lo - a:hi - a]
            ne = exp != self.buf[c0:c1]
            n = int(ne.sum().item())
            if n and first is None:
                first = c0 + int(torch.argmax(ne.view(torch.uint8)).item())
                was, now = int(exp[first - c0].item()), int(self.buf[first].item())
            count += n
            del ne
        if count:
            region, row, col = self._region(first)
            raise GuardError(region, row, col, was, now, count, self.name)


def wide_guarded(shape, dtype, layout, seed, name=None, pitch=None):
    """A device mat of `shape` ((h, w) or (h, w, c)) and `dtype` in one of LAYOUTS."""
    return WideGuarded(shape, dtype, layout, seed, name, pitch)


def wide_guarded_like(array, layout, seed, name=None, pitch=None):
    a = np.asarray(array)
    return WideGuarded(a.shape, a.dtype, layout, seed, name, pitch).set(a)
