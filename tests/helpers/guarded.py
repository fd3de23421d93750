"""A mat inside a guard band: the strided view a test hands to the library lies inside ONE larger byte buffer - guard rows above and
below it, a lead of guard bytes before and a pad after every row, one more run after the last row - whose every byte comes from a seeded
generator (never a constant: a stray store of 0, 255 or any fill value shows).  check() compares the whole buffer with the snapshot
taken just before the call and names the first byte that changed where nothing may be written.

    g = guarded((h, w, 3), np.uint8, "device", "odd", seed)     # an output: random bytes in the view as well
    g.set(array)                                                 # an input / in-place mat: the view's content, then a fresh snapshot
    lib.isx_...(as_mat(g.view)); synchronise
    g.check()                      # an output: only the view may have changed
    g.check(written=(c0, c1))      # ... only the columns [c0, c1) of it (or a boolean (h, w) array of the pixels)
    g.check(written=NOTHING)       # a const input: not one byte of the buffer

Layouts (the library picks its store path from pointer and pitch alignment):
    "odd"      first byte element-aligned but not 4-byte aligned (1-byte elements) / not 16-byte aligned (wider ones); the pitch no
               multiple of 4 / of 16
    "aligned"  first byte 256-byte aligned, the pitch a multiple of 64 (an odd one): the dword and vector store path
"""
import numpy as np

LAYOUTS = ("odd", "aligned")
NOTHING = "nothing"          # check(written=NOTHING): the call may not have written the mat at all
ROWS_ABOVE, ROWS_BELOW = 3, 2
TAIL = 96                    # guard bytes after the last guard row
_SLACK = 512                 # room to place the view's first byte at the wanted address


class GuardError(AssertionError):
    """A byte outside what the call may write has changed.  .region is above | below | lead | pad | view."""

    def __init__(self, region, row, col, was, now, count, name):
        super().__init__("%s: %d byte(s) changed outside what the call may write; the first at buffer row %d, byte column %d (%s): "
                         "%d -> %d" % (name or "guarded mat", count, row, col, region, was, now))
        self.region, self.row, self.col = region, row, col


def _torch():
    import torch
    return torch


class Guarded:
    def __init__(self, shape, dtype, where, layout, seed, name=None):
        assert where in ("host", "device") and layout in LAYOUTS and len(shape) in (2, 3)
        self.shape = tuple(int(v) for v in shape)
        self.dtype = np.dtype(dtype)
        self.where, self.layout, self.name = where, layout, name
        h, w = self.shape[:2]
        cn = self.shape[2] if len(self.shape) == 3 else 1
        es = self.dtype.itemsize
        self.row_bytes = w * cn * es
        if layout == "odd":
            unit = 4 if es == 1 else 16
            lead = 5 * es                                   # 5, 10 or 20: element-aligned, and neither 4- nor 16-byte aligned
            pitch = lead + self.row_bytes + 3 * es
            while pitch % unit == 0:
                pitch += es
            first = _SLACK // 2
            while (first + ROWS_ABOVE * pitch + lead) % unit == 0 or (first + ROWS_ABOVE * pitch + lead) % es:
                first += 1
        else:
            lead = 64
            pitch = (lead + self.row_bytes + 7 + 63) // 64 * 64
            if pitch // 64 % 2 == 0:
                pitch += 64                                 # an odd multiple of 64: not every row 128-byte aligned
            first = (-(ROWS_ABOVE * pitch + lead)) % 256    # (relative to a 256-byte aligned base)
        self.lead, self.pitch, self.first = lead, pitch, first
        self.rows = ROWS_ABOVE + h + ROWS_BELOW
        self.nbytes = first + self.rows * pitch + TAIL
        self.offset = first + ROWS_ABOVE * pitch + lead     # of the view's first byte
        fill = np.random.default_rng(seed).integers(0, 256, self.nbytes, dtype=np.uint8)
        if where == "host":
            raw = np.empty(self.nbytes + 256, np.uint8)
            base = (-raw.ctypes.data) % 256
            self._raw = raw                                 # keeps the allocation alive
            self.buf = raw[base:base + self.nbytes]
            self.buf[...] = fill
            self.view = np.ndarray(self.shape, self.dtype, buffer=self.buf, offset=self.offset,
                                   strides=(pitch, cn * es, es) if len(self.shape) == 3 else (pitch, es))
            address = self.view.ctypes.data
        else:
            torch = _torch()
            raw = torch.empty(self.nbytes + 256, dtype=torch.uint8, device="cuda")
            base = (-raw.data_ptr()) % 256
            self._raw = raw
            self.buf = raw[base:base + self.nbytes]
            self.buf.copy_(torch.from_numpy(fill))
            span = (h - 1) * pitch + self.row_bytes if h > 0 else 0
            flat = self.buf[self.offset:self.offset + span].view(getattr(torch, self.dtype.name))
            strides = (pitch // es, cn, 1) if len(self.shape) == 3 else (pitch // es, 1)
            self.view = flat.as_strided(self.shape, strides)
            address = self.view.data_ptr()
        if layout == "odd":
            assert address % es == 0 and address % (4 if es == 1 else 16) != 0 and pitch % (4 if es == 1 else 16) != 0 and pitch % es == 0
        else:
            assert address % 256 == 0 and pitch % 64 == 0
        self.snapshot()

    # ---- content ---------------------------------------------------------------------------------------------------------------
    def snapshot(self):
        """Remember the whole buffer as it is now; check() compares with this."""
        self._snap = self.buf.copy() if self.where == "host" else self.buf.clone()
        return self

    def set(self, array):
        """The view's content (a NumPy array of the view's shape), then a fresh snapshot."""
        a = np.ascontiguousarray(np.asarray(array), self.dtype).reshape(self.shape)
        if self.where == "host":
            self.view[...] = a
        else:
            self.view.copy_(_torch().from_numpy(a))
        return self.snapshot()

    def get(self):
        """A NumPy copy of the view."""
        return self.view.copy() if self.where == "host" else self.view.cpu().numpy()

    # ---- the check -------------------------------------------------------------------------------------------------------------
    def _may_change(self, written):
        """Boolean per byte of the buffer: True where the call may write."""
        h, w = self.shape[:2]
        px = self.row_bytes // w if w else 0                # bytes per pixel
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
        free = np.zeros(self.nbytes, bool)
        rows = free[self.first:self.first + self.rows * self.pitch].reshape(self.rows, self.pitch)
        rows[ROWS_ABOVE:ROWS_ABOVE + h, self.lead:self.lead + self.row_bytes] = np.repeat(m, px, axis=1)
        return free

    def _region(self, i):
        h = self.shape[0]
        row, col = divmod(i - self.first, self.pitch) if i >= self.first else (-1, i)
        if row < ROWS_ABOVE:
            return "above", row, col
        if row >= ROWS_ABOVE + h:
            return "below", row, col
        if col < self.lead:
            return "lead", row, col
        if col >= self.lead + self.row_bytes:
            return "pad", row, col
        return "view", row, col

    def check(self, written=None):
        """Raises GuardError when a byte of the buffer outside `written` differs from the snapshot.  written: None = the whole view may
        have changed; (c0, c1) = its columns [c0, c1); a boolean (h, w) array = those pixels; NOTHING = no byte at all."""
        free = self._may_change(written)
        if self.where == "host":
            bad = (self.buf != self._snap) & ~free
            n = int(bad.sum())
            if not n:
                return
            i = int(np.argmax(bad))
            was, now = int(self._snap[i]), int(self.buf[i])
        else:
            torch = _torch()
            bad = (self.buf != self._snap) & ~torch.from_numpy(free).to(self.buf.device)
            n = int(bad.sum().item())
            if not n:
                return
            i = int(bad.nonzero()[0].item())
            was, now = int(self._snap[i].item()), int(self.buf[i].item())
        region, row, col = self._region(i)
        raise GuardError(region, row, col, was, now, n, self.name)


def guarded(shape, dtype, where, layout, seed, name=None):
    """A mat of `shape` ((h, w) or (h, w, c)) and `dtype` inside a guard band, on the host (NumPy) or the device (torch, cuda)."""
    return Guarded(shape, dtype, where, layout, seed, name)


def guarded_like(array, where, layout, seed, name=None):
    """guarded(...) of the array's shape and type, holding the array."""
    a = np.asarray(array)
    return Guarded(a.shape, a.dtype, where, layout, seed, name).set(a)
