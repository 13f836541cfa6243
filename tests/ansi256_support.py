"""What the tests of the texts in the xterm 256-colour palette share: a reader of the two formats written here from their description
(include/trt_hip.h) -- the home prefix, then cells matched by a regular expression, then row ends, with nothing else -- the palette search
over frames and over every colour, frames made of the colours at which the palette map can go wrong, and device buffers with guards."""
import functools
import re

import numpy as np

from support import GUARD, STORE, DeviceBytes, same_text  # noqa: F401 -- the 256-colour tests take the scaffold from here
from terminalraytracer_amd import host

HOME, END = b"\033[0;0H", b"\033[0m\n"
CELL = {False: re.compile(rb"\033\[48;5;(\d{3})m  "), True: re.compile(rb"\033\[38;5;(\d{3});48;5;(\d{3})m\xe2\x96\x80")}
CELL_BYTES = {False: 13, True: 23}
WIDTHS = (1, 2, 3, 5, 40, 55, 56, 57, 58, 59, 60, 61, 63, 64, 65, 67, 130)
ROWS = (1, 2, 3, 13)


def length(w, h, half):
    return 6 + (23 * w + 5) * ((h + 1) // 2) if half else 6 + (13 * w + 5) * h


def read(text, half):
    """the palette indices a text shows, int [text rows, width] or, of half-block cells, [text rows, width, 2] (upper, lower); raises
    AssertionError on anything that is not prefix, cells, row ends"""
    data = bytes(np.asarray(text, dtype=np.uint8).tobytes()) if not isinstance(text, bytes) else text
    assert data.startswith(HOME), "no home prefix"
    at, rows = len(HOME), []
    while at < len(data):
        row = []
        m = CELL[half].match(data, at)
        while m:
            row.append([int(g) for g in m.groups()])
            at = m.end()
            m = CELL[half].match(data, at)
        assert row, f"byte {at}: no cell"
        assert data.startswith(END, at), f"byte {at}: neither a cell nor a row's end"
        at += len(END)
        rows.append(row)
    assert rows and len({len(r) for r in rows}) == 1, "rows of different widths, or none"
    out = np.array(rows)
    return out if half else out[..., 0]


def frame_indices(shown, rows, half):
    """the indices of the frame's pixels [rows, width] from read()'s cells, and what stands below the last row of an odd half-block frame"""
    if not half:
        return shown, None
    both = np.stack([shown[..., 0], shown[..., 1]], axis=1).reshape(2 * shown.shape[0], shown.shape[1])
    return both[:rows], (both[rows] if rows % 2 else None)


def search(rgb):
    """trt_xterm256_index_search of every pixel of a frame [rows, width, 3]"""
    a = np.asarray(rgb)
    return np.array([[host.xterm256_index_search(int(p[0]), int(p[1]), int(p[2])) for p in row] for row in a])


@functools.lru_cache(maxsize=None)
def search_table():
    """trt_xterm256_index_search of all 2^24 colours, uint8 [2^24], colour r | g << 8 | b << 16 at its own index: read from the texts the host
    emitter, which searches, makes of strips of all colours.  Computed once, never written to."""
    table = np.empty(1 << 24, dtype=np.uint8)
    strip = 1 << 20
    for first in range(0, 1 << 24, strip):
        c = np.arange(first, first + strip, dtype=np.uint32)
        rgb = np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=1).astype(np.uint8).reshape(1, strip, 3)
        cells = host.emitter_ansi256_rgb8(rgb)[6:6 + 13 * strip].reshape(strip, 13)
        assert (cells[:, 6] == ord(";")).all() and (cells[:, 10] == ord("m")).all()
        digits = cells[:, 7:10].astype(np.int32) - ord("0")
        table[first:first + strip] = digits[:, 0] * 100 + digits[:, 1] * 10 + digits[:, 2]
    table.flags.writeable = False
    return table


# the bytes at which a channel changes its cube level or lies on a midpoint, either side of each, and the ends
EDGES = (0, 1, 4, 5, 8, 13, 18, 47, 48, 94, 95, 96, 114, 115, 116, 135, 154, 155, 156, 175, 194, 195, 196, 215, 234, 235, 236, 238, 246, 247, 254, 255)


def edge_frame(w, h, seed):
    """a frame of tie and threshold colours only: every grey (v, v, v) in turn -- the cube against the ramp, and the ramp's own half-way
    points -- between pixels whose channels are drawn from EDGES"""
    rng = np.random.default_rng(seed)
    rgb = rng.choice(np.array(EDGES, dtype=np.uint8), size=(h, w, 3))
    flat = rgb.reshape(-1, 3)
    grey = (np.arange(flat.shape[0]) * 7 + seed) % 256
    every_other = np.arange(flat.shape[0]) % 2 == 0
    flat[every_other] = grey[every_other, None].astype(np.uint8)
    return rgb


def upload_odd(rgb):
    """a frame's bytes in device memory one byte behind an aligned address: (tensor to keep alive, pointer)"""
    import torch
    flat = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)
    src = torch.zeros(flat.size + 1, dtype=torch.uint8, device="cuda:0")
    src[1:] = torch.from_numpy(flat).to("cuda:0")
    torch.cuda.synchronize()
    return src, src.data_ptr() + 1

