"""The delta text on the host (trt_emitter_delta_rgb8, csrc/host/trt_emit.c), without a GPU.  The reference has no such emitter, so the pin is
what a terminal shows: a model of one (ansi_delta_support.Terminal) that has been fed the reference's screenbuffer of frame 0 -- the host
emitter's full text -- and then the delta texts of frames 1..3 shows, cell for cell and in both columns of every cell, the colours of
T.oracle_rgb8 of frame k, none of them the terminal's default background.  The lengths for the demo scene's orbit are the ones a numpy
prototype of the format gave before this code existed."""
import numpy as np
import pytest

import ansi_delta_support as D
from terminalraytracer_amd import host


def _replay(frames, what):
    """frame 0 as the full text, the others as deltas; the terminal shows every frame in its turn.  Returns the deltas' lengths."""
    rows, w, _ = frames[0].shape
    term = D.Terminal(w, rows).feed(D.full_text(frames[0]))
    term.shows(frames[0], f"{what}, the full text of frame 0")
    lengths = []
    for k in range(1, len(frames)):
        text = host.emitter_delta_rgb8(frames[k - 1], frames[k])
        assert text.size <= D.bound(w, rows), (what, k, text.size)
        assert not (text == 0).any() and not (text == 10).any(), f"{what}: a NUL or a newline in a delta text"
        term.feed(text)
        term.shows(frames[k], f"{what}, after the delta {k - 1} -> {k}")
        lengths.append(int(text.size))
    return lengths


def test_the_terminal_shows_the_oracles_orbit_after_every_delta():
    """demo scene, `colors` cubemap, 160 x 48, 10 bounces, 10 rays per pixel, cameras 0..3 of cameras_anim.npz: 66 819 and 66 497 bytes for
    0 -> 1 and 1 -> 2, about a third of the 192 057 of the full text"""
    frames = [D.oracle_rgb("demo", "colors", 160, 48, k, 10, 10) for k in range(4)]
    lengths = _replay(frames, "demo orbit")
    assert lengths[:2] == [66819, 66497], lengths
    assert all(n < 0.84 * 192057 for n in lengths), lengths


@pytest.mark.parametrize("family", D.FAMILIES)
def test_the_terminal_shows_every_pattern_family(family):
    """shown -> next -> shown -> next' over sizes with one cell, one column, one row, odd widths and the demo's: the bound is reached exactly
    where everything changed and all neighbours differ, equal frames give no text"""
    for w, rows in ((1, 1), (2, 1), (1, 3), (7, 3), (65, 3), (160, 48)):
        shown, nxt = D.pair(family, w, rows)
        _, again = D.pair(family, w, rows, seed=1)
        lengths = _replay([shown, nxt, shown, again], f"{family} {w}x{rows}")
        changed = int((shown != nxt).any(axis=2).sum())
        if family == "nothing":
            assert lengths[0] == 0 and changed == 0
        elif family == "all different":
            assert lengths[0] == D.bound(w, rows) and changed == w * rows
        elif family == "all one colour":
            assert lengths[0] == rows * (14 + 19 + 2 * w + 4)
        elif family in ("first only", "last only"):
            assert lengths[0] == 39 and changed == 1
        elif family == "across rows" and w >= 5 and rows > 1:
            assert lengths[0] == 2 * (rows - 1) * (14 + 19 + 4 + 4)  # a cursor address and a colour sequence either side of every row boundary
        elif family == "left colour":
            assert lengths[0] == 39 * changed  # lone cells: the colour is sent although the cell to the left shows it


def test_the_emitter_refuses_what_it_cannot_write():
    a = np.zeros((1, 1, 3), dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    import ctypes as C
    n = C.c_size_t(7)
    lib, ARGUMENT = host.lib(), -106
    args = lambda **k: [k.get("shown", a.ctypes.data), k.get("nxt", a.ctypes.data), k.get("w", 1), k.get("rows", 1), k.get("text", out.ctypes.data),
                        k.get("cap", 39), k.get("n", C.byref(n))]
    assert lib.trt_emitter_delta_rgb8(*args()) == 0 and n.value == 0
    for bad in (dict(shown=None), dict(nxt=None), dict(text=None), dict(n=None), dict(w=0), dict(rows=0), dict(w=-1), dict(w=50000, cap=1 << 30),
                dict(rows=100000, cap=1 << 30), dict(cap=38)):
        assert lib.trt_emitter_delta_rgb8(*args(**bad)) == ARGUMENT, bad
    assert not out.any()
