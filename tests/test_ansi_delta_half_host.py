"""The delta text in half-block cells on the host (trt_emitter_delta_half_rgb8, csrc/host/trt_emit.c), without a GPU.  The reference has no
such emitter, so the pin is what a terminal shows: a model of one (ansi_delta_half_support.Terminal) that has been fed the half-block
keyframe of frame 0 -- host.emitter_half_rgb8's text -- and then the delta texts of frames 1..3 shows, cell for cell and in both halves of
every cell, the colours of T.oracle_rgb8 of frame k, none of them the terminal's default.  Two literals pin which half is which and the
shapes of the records."""
import ctypes as C

import numpy as np
import pytest

import ansi_delta_half_support as H
import ansi_delta_support as D
from terminalraytracer_amd import host

GLYPH = b"\xe2\x96\x80"


def _replay(frames, what):
    """frame 0 as the half-block keyframe, the others as deltas; the terminal shows every frame in its turn.  Returns the deltas' lengths."""
    rows, w, _ = frames[0].shape
    key = host.emitter_half_rgb8(frames[0])
    assert key.size == H.whole_bytes(w, rows)
    term = H.Terminal(w, rows).feed(key)
    term.shows(frames[0], f"{what}, the keyframe of frame 0")
    lengths = []
    for k in range(1, len(frames)):
        text = host.emitter_delta_half_rgb8(frames[k - 1], frames[k])
        assert text.size <= H.bound(w, rows), (what, k, text.size)
        assert not (text == 0).any() and not (text == 10).any(), f"{what}: a NUL or a newline in a delta text"
        term.feed(text)
        term.shows(frames[k], f"{what}, after the delta {k - 1} -> {k}")
        lengths.append(int(text.size))
    return lengths


def test_the_one_cell_spelled_out():
    """1 x 1, (0, 0, 0) -> (1, 2, 3): the pixel is the upper half, the foreground; behind the odd frame the lower half is black"""
    shown, nxt = np.zeros((1, 1, 3), dtype=np.uint8), np.array([[[1, 2, 3]]], dtype=np.uint8)
    want = b"\033[00001;00001H\033[38;2;001;002;003;48;2;000;000;000m\xe2\x96\x80\033[0m"
    assert len(want) == 57 and H.expected(shown, nxt) == want
    assert H.expected(nxt, nxt) == b""


def test_three_cells_spelled_out():
    """3 x 2, all three cells change: cell 1 keeps cell 0's upper colour with another lower one, cell 2 keeps both of cell 1's colours:
    53 + 22 + 7 = 82 bytes"""
    shown = np.zeros((2, 3, 3), dtype=np.uint8)
    nxt = np.array([[[1, 2, 3], [1, 2, 3], [1, 2, 3]], [[4, 5, 6], [7, 8, 9], [7, 8, 9]]], dtype=np.uint8)
    want = (b"\033[00001;00001H\033[38;2;001;002;003;48;2;004;005;006m" + GLYPH + b"\033[48;2;007;008;009m" + GLYPH + GLYPH + b"\033[0m")
    assert len(want) == 82 and H.expected(shown, nxt) == want
    # the converse single colour: the lower one kept, the upper one another
    nxt2 = np.array([[[1, 2, 3], [9, 9, 9]], [[4, 5, 6], [4, 5, 6]]], dtype=np.uint8)
    want2 = b"\033[00001;00001H\033[38;2;001;002;003;48;2;004;005;006m" + GLYPH + b"\033[38;2;009;009;009m" + GLYPH + b"\033[0m"
    assert H.expected(np.zeros((2, 2, 3), dtype=np.uint8), nxt2) == want2
    # a run that starts in column 3 of text row 2: the cursor counts one-column cells and text rows
    shown3 = np.zeros((4, 4, 3), dtype=np.uint8)
    nxt3 = shown3.copy()
    nxt3[3, 2] = (255, 34, 12)
    assert H.expected(shown3, nxt3) == b"\033[00002;00003H\033[38;2;000;000;000;48;2;255;034;012m" + GLYPH + b"\033[0m"


@pytest.mark.parametrize("h", [48, 47])
def test_the_terminal_shows_the_oracles_orbit_after_every_delta(h):
    """demo scene, `colors` cubemap, 160 x 48 and 160 x 47 (an odd frame: the last text row's lower halves stay black), 10 bounces, 10 rays
    per pixel, cameras 0..3 of cameras_anim.npz"""
    frames = [D.oracle_rgb("demo", "colors", 160, h, k, 10, 10) for k in range(4)]
    lengths = _replay(frames, f"demo orbit 160x{h}")
    print(f"160x{h}: delta texts of {lengths} bytes, the whole half-block text has {H.whole_bytes(160, h)}")
    assert all(0 < n <= H.bound(160, h) for n in lengths), lengths


@pytest.mark.parametrize("family", H.FAMILIES)
def test_the_terminal_shows_every_pattern_family(family):
    """shown -> next -> shown -> next' over sizes with one cell, one column, one text row, odd and even frames, odd widths and the demo's:
    the bound is reached exactly where everything changed and both colours differ from the left neighbour's, equal frames give no text"""
    for w, rows in ((1, 1), (2, 1), (1, 2), (1, 3), (7, 3), (7, 4), (65, 5), (160, 47), (160, 48)):
        if family in H.OWN_FAMILIES and w * rows > 1000:
            continue  # these are built a pixel at a time; the C program walks them at the large sizes
        shown, nxt = H.pair(family, w, rows)
        _, again = H.pair(family, w, rows, seed=1)
        lengths = _replay([shown, nxt, shown, again], f"{family} {w}x{rows}")
        trows, even = (rows + 1) // 2, rows % 2 == 0
        run = 14 + 36 + 19 * (w - 1) + 3 * w + 4  # a text row as one run in which every cell but the first sets one colour
        if family == "nothing":
            assert lengths[0] == 0
        elif family == "all different":
            assert lengths[0] == H.bound(w, rows) - (0 if even else 17 * (w - 1))  # an odd frame's last text row has one lower colour
        elif family == "all one colour":
            assert lengths[0] == trows * (14 + 36 + 3 * w + 4)
        elif family in ("first only", "last only"):
            assert lengths[0] == 57
        elif family in ("same upper", "same lower") and even:
            assert lengths[0] == trows * run
        elif family == "upper only":
            assert lengths[0] >= trows * run
        elif family == "lower only":
            assert lengths[0] >= (rows // 2) * run and (rows > 1 or lengths[0] == 0)


def test_the_size_pins():
    from terminalraytracer_amd import hip
    assert hip.ansi_delta_half_capacity(1, 1) == 57
    assert hip.ansi_delta_half_capacity(160, 48) == hip.ansi_delta_half_capacity(160, 47) == 150192
    assert hip.ansi_delta_half_capacity(100000, 1) == hip.ansi_delta_half_capacity(1, 199999) == hip.ansi_delta_half_capacity(0, 1) == 0
    assert hip.ansi_delta_half_capacity(99999, 199998) == 99999 * (39 * 99999 + 18)
    lib = host.lib()
    out, n = np.zeros(1 << 20, dtype=np.uint8), C.c_size_t(0)
    # the bound is the capacity: reached by 1 x 1, and one byte below it refused
    a, b = np.zeros((1, 1, 3), dtype=np.uint8), np.ones((1, 1, 3), dtype=np.uint8)
    assert lib.trt_emitter_delta_half_rgb8(a.ctypes.data, b.ctypes.data, 1, 1, out.ctypes.data, 57, C.byref(n)) == 0 and n.value == 57
    for w, rows, want in ((1, 1, 57), (160, 48, 150192), (160, 47, 150192)):
        assert H.bound(w, rows) == want and H.bound(w, rows) > H.whole_bytes(w, rows)
        shown, nxt = H.pair("all different", w, rows)
        assert lib.trt_emitter_delta_half_rgb8(shown.ctypes.data, nxt.ctypes.data, w, rows, out.ctypes.data, want, C.byref(n)) == 0
        assert lib.trt_emitter_delta_half_rgb8(shown.ctypes.data, nxt.ctypes.data, w, rows, out.ctypes.data, want - 1, C.byref(n)) == -106


def test_the_emitter_refuses_what_it_cannot_write():
    a = np.zeros((1, 1, 3), dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    n = C.c_size_t(7)
    lib, ARGUMENT = host.lib(), -106
    args = lambda **k: [k.get("shown", a.ctypes.data), k.get("nxt", a.ctypes.data), k.get("w", 1), k.get("rows", 1), k.get("text", out.ctypes.data),
                        k.get("cap", 57), k.get("n", C.byref(n))]
    assert lib.trt_emitter_delta_half_rgb8(*args()) == 0 and n.value == 0
    for bad in (dict(shown=None), dict(nxt=None), dict(text=None), dict(n=None), dict(w=0), dict(rows=0), dict(w=-1), dict(w=100000, cap=1 << 30),
                dict(rows=199999, cap=1 << 30), dict(cap=56)):
        assert lib.trt_emitter_delta_half_rgb8(*args(**bad)) == ARGUMENT, bad
    assert not out.any()
