"""What the tests of the delta text in half-block cells share (test_ansi_delta_half_host.py without a GPU, test_ansi_delta_half_text.py
with one): a small model of a terminal that shows half-block cells, and the families of frame pairs the format is exercised with.
Expected texts never come from the library's device route: they are host.emitter_delta_half_rgb8 (the sequential C statement) of pattern
frames or of T.oracle_rgb8 frames, keyframes host.emitter_half_rgb8's, and what the model shows is held against the frames themselves."""
import re

import numpy as np

import ansi_delta_support as D
from terminalraytracer_amd import hip, host

DEFAULT = -2   # after "\033[0m": the terminal's own colour
NEVER = -1     # a half cell nothing was painted on

_TOKEN = re.compile(rb"\x1b\[(\d*);(\d*)H"
                    rb"|\x1b\[38;2;(\d+);(\d+);(\d+);48;2;(\d+);(\d+);(\d+)m"
                    rb"|\x1b\[38;2;(\d+);(\d+);(\d+)m"
                    rb"|\x1b\[48;2;(\d+);(\d+);(\d+)m"
                    rb"|(\x1b\[0m)|(\xe2\x96\x80)|(\n)")


def _colour(at, groups):
    r, g, b = (int(x) for x in groups)
    assert max(r, g, b) <= 255, (at, r, g, b)
    return r | g << 8 | b << 16


class Terminal:
    """cursor, current foreground, current background, a grid of (upper, lower) per one-column cell.  It understands exactly what the two
    half-block emitters write -- ESC[r;cH (a parameter 0 or empty counts as 1), the 36-byte double colour, the two 19-byte single colours,
    ESC[0m, the glyph U+2580, newline -- and fails on anything else, on a glyph outside the screen, on a glyph painted while either colour is
    the terminal's default, and on a colour component above 255."""

    def __init__(self, width, rows):
        self.width, self.rows, self.trows = width, rows, (rows + 1) // 2
        self.grid = np.full((self.trows, width, 2), NEVER, dtype=np.int64)
        self.row = self.col = 0
        self.foreground = self.background = DEFAULT

    def feed(self, text):
        data = bytes(np.asarray(text, dtype=np.uint8).tobytes()) if not isinstance(text, (bytes, bytearray)) else bytes(text)
        at = 0
        while at < len(data):
            m = _TOKEN.match(data, at)
            assert m, f"byte {at} of {len(data)}: the terminal model does not know {data[at:at + 12]!r}"
            g = m.groups()
            if g[0] is not None:
                self.row, self.col = max(int(g[0] or 1), 1) - 1, max(int(g[1] or 1), 1) - 1
            elif g[2] is not None:
                self.foreground, self.background = _colour(at, g[2:5]), _colour(at, g[5:8])
            elif g[8] is not None:
                self.foreground = _colour(at, g[8:11])
            elif g[11] is not None:
                self.background = _colour(at, g[11:14])
            elif g[14] is not None:
                self.foreground = self.background = DEFAULT
            elif g[15] is not None:
                assert self.row < self.trows and self.col < self.width, f"byte {at}: a glyph at row {self.row}, column {self.col} of a {self.trows} x {self.width} screen"
                assert self.foreground != DEFAULT and self.background != DEFAULT, f"byte {at}: a glyph in the terminal's default colours at ({self.row}, {self.col})"
                self.grid[self.row, self.col] = (self.foreground, self.background)
                self.col += 1
            else:
                self.row, self.col = self.row + 1, 0
            at = m.end()
        return self

    def shows(self, rgb, what=""):
        """every cell shows the frame rgb [rows, width, 3]: row 2 t in its upper half, row 2 t + 1 (black behind an odd frame) in its lower"""
        rows, width, _ = rgb.shape
        assert (rows, width) == (self.rows, self.width)
        padded = np.zeros((2 * self.trows, width, 3), dtype=np.int64)
        padded[:rows] = rgb
        want = (padded[..., 0] | padded[..., 1] << 8 | padded[..., 2] << 16).reshape(self.trows, 2, width).transpose(0, 2, 1)
        wrong = self.grid != want
        if wrong.any():
            t, c, h = np.argwhere(wrong)[0]
            kind = {DEFAULT: "the default colour", NEVER: "nothing"}.get(int(self.grid[t, c, h]), f"{int(self.grid[t, c, h]):06x}")
            raise AssertionError(f"{what}: {int(wrong.sum())} half cells show another colour; cell ({t}, {c}) shows {kind} in its {('upper', 'lower')[h]} half "
                                 f"for {int(want[t, c, h]):06x}")


def bound(w, rows):
    return ((rows + 1) // 2) * (39 * w + 18)


def whole_bytes(w, rows):
    return 6 + (39 * w + 5) * ((rows + 1) // 2)


# ---- frame pairs: the delta text's families over the pixels, and those that make every record length of this format ----

OWN_FAMILIES = ("upper only", "lower only", "same upper", "same lower")
FAMILIES = D.FAMILIES + OWN_FAMILIES


def _row_all_different(rng, shown, nxt, r):
    w = shown.shape[1]
    for c in range(w):  # different from the shown colour and from the new colour to the left
        nxt[r, c] = D._other(rng, (1,), shown[r, c][None], (nxt[r, c - 1] if c else shown[r, c])[None])[0]


def _row_all_one(shown, nxt, r):
    shown[r] = (0x10, 0x20, 0x30)
    shown[r, ::2, 0] = 0x11
    nxt[r] = (0xa0, 0xb0, 0xc0)


def pair(family, w, rows, seed=0):
    """(shown, next): two frames of bytes [rows, w, 3] of the family.  "all one colour" is the family in which both colours equal the left
    neighbour's (records of 3 and 7 bytes); "all different" reaches the bound in an even frame."""
    if family in D.FAMILIES:
        return D.pair(family, w, rows, seed)
    rng = np.random.default_rng([seed, 100 + OWN_FAMILIES.index(family), w, rows])
    shown = rng.integers(0, 256, (rows, w, 3), dtype=np.uint8)
    nxt = shown.copy()
    for r in range(rows):
        lower = r & 1
        if family == "upper only" and not lower or family == "lower only" and lower:
            _row_all_different(rng, shown, nxt, r)
        elif family == "same upper":  # the upper rows to one colour, the lower ones all different
            _row_all_different(rng, shown, nxt, r) if lower else _row_all_one(shown, nxt, r)
        elif family == "same lower":
            _row_all_one(shown, nxt, r) if lower else _row_all_different(rng, shown, nxt, r)
    return np.ascontiguousarray(shown), np.ascontiguousarray(nxt)


def expected(shown, nxt):
    """the sequential emitter's text of the pair, as bytes"""
    return host.emitter_delta_half_rgb8(shown, nxt).tobytes()


def render_half(ctx, cam, rows, offset=0, what=""):
    return D.render_text(ctx, hip.Context.render_device_ansi_delta_half, hip.ansi_delta_half_capacity, cam, rows, offset, what)


HALF = D.Kind(host.emitter_half_rgb8, host.emitter_delta_half_rgb8, Terminal, render_half)
