"""tests/helpers/guarded.py on the host: every layout and type gives the alignment it promises, as_mat() sees the view and not the buffer,
a stray store anywhere in the guard band (or in the view outside `written`) is found and its region named, and a call that writes only
where it may passes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import guarded as G  # noqa: E402
from imagestitch_amd import _lib  # noqa: E402

TYPES = [(np.uint8, 1), (np.uint8, 3), (np.int16, 3), (np.int32, 1), (np.float32, 1), (np.float32, 3)]
SHAPES = [(1, 1), (3, 5), (5, 67)]


def _make(dtype, cn, layout, hw=(5, 67), seed=3):
    shape = hw if cn == 1 else hw + (cn,)
    return G.guarded(shape, dtype, "host", layout, seed)


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("dtype,cn", TYPES)
def test_layout_and_as_mat(dtype, cn, layout):
    for hw in SHAPES:
        g = _make(dtype, cn, layout, hw)
        es = np.dtype(dtype).itemsize
        m = _lib.as_mat(g.view)
        assert m.data == g.buf.ctypes.data + g.offset and m.data == g.view.ctypes.data      # the view's pointer, not the buffer's
        assert m.step == g.pitch and m.step != hw[1] * cn * es
        assert (m.rows, m.cols, m.device) == (hw[0], hw[1], -1)
        assert m.type == _lib._NP_TYPES[(np.dtype(dtype).name, cn)]
        if layout == "odd":
            unit = 4 if es == 1 else 16
            assert m.data % es == 0 and m.data % unit != 0 and m.step % unit != 0 and m.step % es == 0
        else:
            assert m.data % 256 == 0 and m.step % 64 == 0
        assert G.ROWS_ABOVE >= 2 and G.ROWS_BELOW >= 2 and g.lead > 0 and g.pitch - g.lead - g.row_bytes > 0 and G.TAIL > 0
        assert g.offset - g.lead == g.first + G.ROWS_ABOVE * g.pitch
        assert g.nbytes == g.first + (hw[0] + G.ROWS_ABOVE + G.ROWS_BELOW) * g.pitch + G.TAIL


def test_the_fill_is_seeded_and_no_constant():
    a, b, c = (G.guarded((4, 9, 3), np.uint8, "host", "odd", s) for s in (1, 1, 2))
    assert np.array_equal(a.buf, b.buf) and not np.array_equal(a.buf, c.buf)
    assert len(np.unique(a.buf)) > 100


def _flip(g, i):
    g.buf[i] ^= 0x5A


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("dtype,cn", TYPES)
def test_stray_stores_are_found_and_named(dtype, cn, layout):
    h, w = 5, 67
    probe = _make(dtype, cn, layout)
    row0 = probe.first + G.ROWS_ABOVE * probe.pitch                     # first byte of the buffer row that holds view row 0
    strays = {
        "the last guard byte of the buffer": (probe.nbytes - 1, "below"),
        "the first byte after a row": (row0 + 2 * probe.pitch + probe.lead + probe.row_bytes, "pad"),
        "the first byte after the last row": (row0 + (h - 1) * probe.pitch + probe.lead + probe.row_bytes, "pad"),
        "the byte before a row": (row0 + 1 * probe.pitch + probe.lead - 1, "lead"),
        "the byte before the view": (row0 + probe.lead - 1, "lead"),
        "the row above the view": (row0 - probe.pitch + probe.lead + 3, "above"),
        "the row below the view": (row0 + h * probe.pitch + probe.lead + 3, "below"),
        "the first byte of the buffer": (0, "above"),
    }
    for what, (i, region) in strays.items():
        for written in (None, G.NOTHING, (0, w)):
            g = _make(dtype, cn, layout)
            _flip(g, i)
            with pytest.raises(G.GuardError) as e:
                g.check(written)
            assert e.value.region == region, (what, e.value.region)
            assert e.value.row == ((i - g.first) // g.pitch if i >= g.first else -1), what
            if i >= g.first:
                assert e.value.col == (i - g.first) % g.pitch, what
            assert region in str(e.value)
    # a stray store of the value that is already there cannot be seen; one of any other value is - a constant would not do
    g = _make(dtype, cn, layout)
    g.buf[row0 - 1] = (int(g.buf[row0 - 1]) + 1) % 256
    with pytest.raises(G.GuardError):
        g.check()


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("dtype,cn", TYPES)
def test_written_limits_the_view(dtype, cn, layout):
    h, w = 5, 67
    rng = np.random.default_rng(5)
    shape = (h, w) if cn == 1 else (h, w, cn)
    new = rng.integers(1, 100, shape).astype(dtype)
    g = _make(dtype, cn, layout)
    g.check(), g.check(G.NOTHING), g.check((3, 9)), g.check(np.zeros((h, w), bool))       # untouched: everything passes
    g.set(new)
    assert np.array_equal(g.get(), new)
    g.check(G.NOTHING)                                                   # set() takes a fresh snapshot
    g.view[...] = new + 1
    g.check()                                                            # written only inside the view
    g.check((0, w)), g.check(np.ones((h, w), bool))
    with pytest.raises(G.GuardError) as e:                               # ... which an input may not be
        g.check(G.NOTHING)
    assert e.value.region == "view" and e.value.row == G.ROWS_ABOVE and 0 <= e.value.col - g.lead < np.dtype(dtype).itemsize
    # a column range: one pixel outside it
    g = _make(dtype, cn, layout)
    g.set(new)
    g.view[:, 64:66] = new[:, 64:66] + 1
    g.check((64, 66)), g.check((0, 66)), g.check((64, 200))
    for rng_ in ((64, 65), (65, 66), (0, 64), (66, 67)):
        with pytest.raises(G.GuardError) as e:
            g.check(rng_)
        assert e.value.region == "view"
    # a pixel mask
    g = _make(dtype, cn, layout)
    g.set(new)
    m = np.zeros((h, w), bool)
    m[2, 5] = m[4, 66] = True
    g.view[2, 5] = new[2, 5] + 1
    g.view[4, 66] = new[4, 66] + 1
    g.check(m)
    g.view[4, 65] = new[4, 65] + 1                                       # an in-view pixel outside `written`
    with pytest.raises(G.GuardError) as e:
        g.check(m)
    px = g.row_bytes // w
    assert e.value.region == "view" and e.value.row == G.ROWS_ABOVE + 4 and g.lead + 65 * px <= e.value.col < g.lead + 66 * px
    # the last byte of a pixel next to `written` (a store one element too wide)
    g = _make(dtype, cn, layout)
    g.set(new)
    g.buf[g.offset + 10 * px - 1] ^= 1
    g.check((0, 10))
    with pytest.raises(G.GuardError):
        g.check((0, 9))
    with pytest.raises(G.GuardError):
        g.check((10, w))


# (layout, pitch or None = the layout's default, rows, on the fast side?) - every mat tests/test_gpu_addressing_limits.py builds
WIDE_CASES = [("wide", None, 8, False), ("wide", (1 << 24) + 64, 24, False), ("wide_below", None, 8, True), ("wide_below", None, 24, True),
              ("tall31", None, 255, True), ("tall31", None, 256, False), ("tall31", None, 257, False),
              ("tall32", None, 511, True), ("tall32", None, 512, False), ("tall32", (1 << 24) - 64, 256, True), ("tall32", (1 << 24) - 64, 257, False)]


@pytest.mark.parametrize("dtype,cn", TYPES)
@pytest.mark.parametrize("layout,pitch,rows,fast", WIDE_CASES)
def test_large_pitch_layout_arithmetic(layout, pitch, rows, fast, dtype, cn):
    """tests/helpers/guarded_wide.py, its arithmetic only (no device): each layout's pitch and row count lie on the stated side of the
    threshold it is named for, the view lies inside the buffer behind the lead and before the tail that keep a truncated, wrapped or
    sign-extended offset inside the allocation, and its first byte and pitch are aligned for the element."""
    from helpers import guarded_wide as W
    es = np.dtype(dtype).itemsize
    for w in (24, 40, 70):
        p = W.plan((rows, w, cn) if cn > 1 else (rows, w), dtype, layout, pitch)
        assert p.rows == rows and p.row_bytes == w * cn * es
        if layout == "wide":
            assert p.pitch >= 1 << 24 and p.pitch in (1 << 24, (1 << 24) + 64) and 8 <= rows <= 24
        elif layout == "wide_below":
            assert (1 << 24) - 64 <= p.pitch < 1 << 24 and (p.pitch == (1 << 24) - 4) == (es * cn == 1)
        if layout.startswith("wide"):
            assert (p.pitch < 1 << 24) == fast and p.pitch * rows < 1 << 31             # only the pitch is past a limit
            assert p.nbytes <= 420 << 20                                                  # "about 400 MiB"
        elif layout == "tall31":
            assert p.pitch == 1 << 23 and (p.pitch * rows < 1 << 31) == fast
            assert p.pitch * 255 < 1 << 31 and p.pitch * 256 == 1 << 31
        else:
            assert p.pitch < 1 << 24 and (p.pitch * rows < 1 << 32) == fast
            if fast:
                assert p.pitch * (rows + 1) >= 1 << 32                                   # the last row count on the fast side
            assert p.pitch * rows >= 1 << 31                                             # past the sources' limit either way
        # the view inside the buffer, behind the lead and before the tail
        lead = (1 << 31) + (64 << 10) if layout.startswith("tall") else 64 << 10
        assert p.offset >= lead and p.span == (rows - 1) * p.pitch + p.row_bytes
        assert p.offset + p.span + (64 << 10) <= p.nbytes
        if layout == "tall32":
            assert p.nbytes >= p.offset + (1 << 32)
        # every offset a fast kernel can get wrong stays inside: the step truncated to 24 bits, the sum wrapped at 2^32, the sum signed
        last = p.span - 1
        for wrong in ((rows - 1) * (p.pitch & 0xFFFFFF) + p.row_bytes - 1, last % (1 << 32), last % (1 << 32) - (1 << 32) if last % (1 << 32) >= 1 << 31 else 0):
            assert 0 <= p.offset + wrong < p.nbytes, (layout, rows, wrong)
        assert p.offset % 256 == 0 and p.offset % es == 0 and p.pitch % es == 0 and p.pitch % 4 == 0
        assert W.bytes_needed((rows, w), dtype, layout, pitch) >= p.nbytes
    with pytest.raises(AssertionError):
        W.plan((8, 24), np.uint8, layout, 12345)                                          # no pitch but the layout's own


def test_guarded_like_holds_the_array():
    a = np.random.default_rng(1).integers(0, 255, (3, 5, 3)).astype(np.int16)
    g = G.guarded_like(a, "host", "aligned", 4)
    assert g.view.dtype == np.int16 and np.array_equal(g.view, a)
    g.check(G.NOTHING)
