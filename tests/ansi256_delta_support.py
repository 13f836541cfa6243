"""What the tests of the delta texts in the xterm 256-colour palette share (test_ansi256_delta_host.py without a GPU,
test_ansi256_delta_text.py and test_ansi256_delta_batch_text.py with one): models of a terminal that keeps palette indices, for both
shapes of cell; the palette's 240 fixed entries and the three families of frame pairs that only a palette text has; and what each kind of
cell supplies to the harness of ansi_delta_support and ansi_delta_batch_support.  Expected texts never come from the library's device
route: they are host.emitter_delta256_rgb8 (the sequential C statement, which SEARCHES the palette) of pattern frames or of T.oracle_rgb8
frames, keyframes host.emitter_ansi256_rgb8's, and what a model shows is held against the search's indices of the frames themselves."""
import functools
import re

import numpy as np

import ansi256_support as P
import ansi_delta_batch_support as S
import ansi_delta_half_support as H
import ansi_delta_support as D
from terminalraytracer_amd import hip, host

DEFAULT = -2   # after "\033[0m": the terminal's own colour
NEVER = -1     # a cell nothing was painted on
BLACK = 16     # the lower index behind an odd half-block frame's last row


def indices(rgb):
    """the palette index of every pixel of a frame [rows, width, 3] BY THE SEARCH: int64 [rows, width], read from the host emitter's whole text"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    return P.read(host.emitter_ansi256_rgb8(rgb), False).astype(np.int64).reshape(rgb.shape[:2])


def half_indices(rgb):
    """(upper, lower) of every half-block cell: int64 [text rows, width, 2], black below an odd frame"""
    idx = indices(rgb)
    rows, width = idx.shape
    padded = np.full((2 * ((rows + 1) // 2), width), BLACK, dtype=np.int64)
    padded[:rows] = idx
    return padded.reshape(-1, 2, width).transpose(0, 2, 1)


_TOKEN = re.compile(rb"\x1b\[(\d*);(\d*)H|\x1b\[48;5;(\d+)m|(\x1b\[0m)|( +)|(\n)")
_HALF_TOKEN = re.compile(rb"\x1b\[(\d*);(\d*)H|\x1b\[38;5;(\d+);48;5;(\d+)m|\x1b\[38;5;(\d+)m|\x1b\[48;5;(\d+)m|(\x1b\[0m)|(\xe2\x96\x80)|(\n)")


def _entry(at, digits):
    n = int(digits)
    assert 16 <= n <= 255, f"byte {at}: palette entry {n}"
    return n


def _data(text):
    return bytes(text) if isinstance(text, (bytes, bytearray)) else bytes(np.asarray(text, dtype=np.uint8).tobytes())


class Terminal:
    """cursor, current background, a grid of column indices (a cell of the picture is two columns wide).  It understands exactly what the
    palette emitters of full cells write -- ESC[r;cH (a parameter 0 or empty counts as 1), ESC[48;5;Nm, ESC[0m, space, newline -- and fails
    on anything else, on a space outside the screen, on a space in the default background and on an entry outside 16..255."""

    def __init__(self, width, rows):
        self.width, self.rows = width, rows
        self.grid = np.full((rows, 2 * width), NEVER, dtype=np.int64)
        self.row = self.col = 0
        self.background = DEFAULT
        self.records = []  # (row, cell) of every pair of spaces painted behind a cursor address: the changed cells of a delta text

    def feed(self, text):
        data, at = _data(text), 0
        while at < len(data):
            m = _TOKEN.match(data, at)
            assert m, f"byte {at} of {len(data)}: the terminal model does not know {data[at:at + 12]!r}"
            if m.group(1) is not None:
                self.row, self.col = max(int(m.group(1) or 1), 1) - 1, max(int(m.group(2) or 1), 1) - 1
            elif m.group(3) is not None:
                self.background = _entry(at, m.group(3))
            elif m.group(4) is not None:
                self.background = DEFAULT
            elif m.group(5) is not None:
                n = len(m.group(5))
                assert self.row < self.rows and self.col + n <= 2 * self.width, f"byte {at}: {n} space(s) at row {self.row}, column {self.col} of a {self.rows} x {2 * self.width} screen"
                assert self.background != DEFAULT, f"byte {at}: a space in the terminal's default background at ({self.row}, {self.col})"
                assert n % 2 == 0 and self.col % 2 == 0, f"byte {at}: {n} space(s) at column {self.col}: half a cell"
                self.grid[self.row, self.col:self.col + n] = self.background
                self.records += [(self.row, c // 2) for c in range(self.col, self.col + n, 2)]
                self.col += n
            else:
                self.row, self.col = self.row + 1, 0
            at = m.end()
        return self

    def shows(self, rgb, what=""):
        """every cell shows the search's index of its pixel of the frame rgb [rows, width, 3], in both of its columns"""
        want = indices(rgb)
        for half in (0, 1):
            got = self.grid[:, half::2]
            wrong = got != want
            if wrong.any():
                r, c = np.argwhere(wrong)[0]
                kind = {DEFAULT: "the default background", NEVER: "nothing"}.get(int(got[r, c]), f"entry {int(got[r, c])}")
                raise AssertionError(f"{what}: {int(wrong.sum())} cells show another entry in column {half}; cell ({r}, {c}) shows {kind} for entry {int(want[r, c])}")


class HalfTerminal:
    """cursor, current foreground AND background, a grid of (upper, lower) indices per one-column cell.  It understands exactly what the
    palette emitters of half-block cells write -- ESC[r;cH, the 20-byte double colour, the two 11-byte single colours, ESC[0m, the glyph
    U+2580, newline -- and fails on anything else, on a glyph outside the screen, on a glyph painted while either colour is the terminal's
    default, and on an entry outside 16..255."""

    def __init__(self, width, rows):
        self.width, self.rows, self.trows = width, rows, (rows + 1) // 2
        self.grid = np.full((self.trows, width, 2), NEVER, dtype=np.int64)
        self.row = self.col = 0
        self.foreground = self.background = DEFAULT
        self.records = []

    def feed(self, text):
        data, at = _data(text), 0
        while at < len(data):
            m = _HALF_TOKEN.match(data, at)
            assert m, f"byte {at} of {len(data)}: the terminal model does not know {data[at:at + 12]!r}"
            g = m.groups()
            if g[0] is not None:
                self.row, self.col = max(int(g[0] or 1), 1) - 1, max(int(g[1] or 1), 1) - 1
            elif g[2] is not None:
                self.foreground, self.background = _entry(at, g[2]), _entry(at, g[3])
            elif g[4] is not None:
                self.foreground = _entry(at, g[4])
            elif g[5] is not None:
                self.background = _entry(at, g[5])
            elif g[6] is not None:
                self.foreground = self.background = DEFAULT
            elif g[7] is not None:
                assert self.row < self.trows and self.col < self.width, f"byte {at}: a glyph at row {self.row}, column {self.col} of a {self.trows} x {self.width} screen"
                assert self.foreground != DEFAULT and self.background != DEFAULT, f"byte {at}: a glyph in the terminal's default colours at ({self.row}, {self.col})"
                self.grid[self.row, self.col] = (self.foreground, self.background)
                self.records.append((self.row, self.col))
                self.col += 1
            else:
                self.row, self.col = self.row + 1, 0
            at = m.end()
        return self

    def shows(self, rgb, what=""):
        """every cell shows the frame rgb [rows, width, 3]: row 2 t's index in its upper half, row 2 t + 1's (black behind an odd frame) in its lower"""
        assert rgb.shape[:2] == (self.rows, self.width)
        want = half_indices(rgb)
        wrong = self.grid != want
        if wrong.any():
            t, c, h = np.argwhere(wrong)[0]
            kind = {DEFAULT: "the default colour", NEVER: "nothing"}.get(int(self.grid[t, c, h]), f"entry {int(self.grid[t, c, h])}")
            raise AssertionError(f"{what}: {int(wrong.sum())} half cells show another entry; cell ({t}, {c}) shows {kind} in its {('upper', 'lower')[h]} half "
                                 f"for entry {int(want[t, c, h])}")


def changed_cells(terminal, w, rows, text):
    """the cells a delta text paints, as a set of (row, column), by a fresh model of the kind"""
    return set(terminal(w, rows).feed(text).records)


def bound(w, rows, half=False):
    return ((rows + 1) // 2) * (23 * w + 18) if half else rows * (13 * w + 13 + 5 * ((w + 1) // 2))


# ---- the palette's 240 fixed entries, from their description, held against the search ----

@functools.lru_cache(maxsize=None)
def entries():
    """uint8 [240, 3]: the colour of entry 16 + i; every one is its own nearest, and so is the colour one off in its red byte"""
    levels = (0, 95, 135, 175, 215, 255)
    table = [(levels[i // 36], levels[i // 6 % 6], levels[i % 6]) for i in range(216)] + [(8 + 10 * k,) * 3 for k in range(24)]
    out = np.array(table, dtype=np.uint8)
    for i, (r, g, b) in enumerate(table):
        assert host.xterm256_index_search(r, g, b) == 16 + i == host.xterm256_index_search(r - 1 if r == 255 else r + 1, g, b), (i, r, g, b)
    out.flags.writeable = False
    return out


def nudged(rgb):
    """other bytes of the same entries: the red byte one off"""
    out = np.array(rgb, dtype=np.uint8)
    red = out[..., 0].astype(np.int64)
    out[..., 0] = np.where(red == 255, 254, red + 1)
    return out


def _other_index(rng, shape, *avoid):
    """random entries 0..239 [shape] that differ, cell by cell, from each of `avoid`"""
    out = rng.integers(0, 240, shape)
    for _ in range(64):
        clash = np.zeros(shape, dtype=bool)
        for a in avoid:
            clash |= out == a
        if not clash.any():
            return out
        out[clash] = rng.integers(0, 240, int(clash.sum()))
    raise AssertionError("no entries found")


OWN_FAMILIES = ("same index", "index run", "longest")
FAMILIES = D.FAMILIES + OWN_FAMILIES          # full cells
HALF_FAMILIES = H.FAMILIES + OWN_FAMILIES     # half-block cells


def pair(family, w, rows, seed=0, half=False):
    """(shown, next): two frames of bytes [rows, w, 3] of the family, for full cells or for half-block cells.
    "same index": every pixel's bytes differ between the frames, no index does, horizontal neighbours have different entries.
    "index run": every pixel changes its entry, a row's new pixels have alternating bytes of ONE entry.
    "longest": what reaches the bound -- full cells: changed and unchanged cells in turn, an even row's last two cells both; half-block
    cells: every pixel another entry than before and than its new left neighbour."""
    if family not in OWN_FAMILIES:
        return H.pair(family, w, rows, seed) if half else D.pair(family, w, rows, seed)
    rng = np.random.default_rng([seed, 200 + OWN_FAMILIES.index(family), w, rows, int(half)])
    colours = entries()
    was = np.empty((rows, w), dtype=np.int64)
    for c in range(w):
        was[:, c] = _other_index(rng, (rows,), was[:, c - 1] if c else -1)
    shown = colours[was]
    if family == "same index":
        nxt = nudged(shown)
    elif family == "index run":
        nxt = colours[np.broadcast_to(_row_entry_outside(rng, was), (rows, w))].copy()
        nxt[:, 1::2] = nudged(nxt[:, 1::2])
    else:
        now = was.copy()
        for c in range(w):
            if half or c % 2 == 0 or c == w - 1:
                now[:, c] = _other_index(rng, (rows,), was[:, c], now[:, c - 1] if c else -1)
        nxt = colours[now]
    return np.ascontiguousarray(shown), np.ascontiguousarray(nxt)


def _row_entry_outside(rng, was):
    """per row an entry that no pixel of the row has, so that every pixel changes: int64 [rows, 1] (a row in which all 240 occur: any other
    than its first pixel's)"""
    out = np.empty((was.shape[0], 1), dtype=np.int64)
    for r, row in enumerate(was):
        free = np.setdiff1d(np.arange(240), row)
        out[r, 0] = rng.choice(free) if free.size else (row[0] + 1) % 240
    return out


# ---- what the kinds of cell supply to the harnesses ----

def render_256(ctx, cam, rows, offset=0, what=""):
    return D.render_text(ctx, hip.Context.render_device_ansi256_delta, hip.ansi256_delta_capacity, cam, rows, offset, what)


def render_256_half(ctx, cam, rows, offset=0, what=""):
    return D.render_text(ctx, functools.partial(hip.Context.render_device_ansi256_delta, half=True), functools.partial(hip.ansi256_delta_capacity, half=True),
                         cam, rows, offset, what)


def _kind(half):
    on = functools.partial
    names = tuple(n.replace("ansi256_delta", "ansi256_delta_half") if half else n
                  for n in ("trt_ansi256_delta_chain_from_rgb8_device", "trt_render_device_batch_ansi256_delta", "trt_render_host_batch_ansi256_delta"))
    return S.Kind(on(host.emitter_ansi256_rgb8, half=half), on(host.emitter_delta256_rgb8, half=half), HalfTerminal if half else Terminal,
                  render_256_half if half else render_256, on(hip.ansi256_delta_capacity, half=half), on(hip.Context.ansi256_delta_chain_from_rgb8, half=half),
                  on(hip.Context.ansi256_delta_chain_kernel_times, half=half), on(hip.Context.render_device_batch_ansi256_delta, half=half),
                  on(hip.Context.render_host_batch_ansi256_delta, half=half), names, on(hip.Context.ansi256_delta_from_rgb8, half=half))


FULL256, HALF256 = _kind(False), _kind(True)
KINDS = {"full256": FULL256, "half256": HALF256}
ALL_KINDS = {"full": S.FULL, "half": S.HALF, **KINDS}  # the four kinds a context's shown frame can have been sent as
