"""What the tests of the DEC sixel image share (csrc/trt_sixel.h): a formatter written from the format's description, with a 240-entry
search of its own for the palette indices, and a STRUCTURAL READER, which stands in for the terminal nobody here has: it takes a text apart
into the home prefix, the DCS introducer, the raster attributes, the 240 colour definitions, the bands' colour rows and the terminator,
asserts every rule of the format on the way, and returns the frame of palette indices the text paints."""
import re

import numpy as np

HOME, DCS, END = b"\033[0;0H", b"\033P0;1;0q", b"\033\\"
FIXED = 4352   # everything but the colour rows
BAND = 6
LEVELS = (0, 95, 135, 175, 215, 255)
PALETTE = np.array([(LEVELS[i], LEVELS[j], LEVELS[k]) for i in range(6) for j in range(6) for k in range(6)] + [(8 + 10 * k,) * 3 for k in range(24)],
                   dtype=np.int64)  # entry 16 + its place


def pad(width):
    return 1 + (-(width + 1)) % 4


def row_bytes(width):
    return 4 + width + pad(width)


def length(width, colour_rows):
    return FIXED + row_bytes(width) * colour_rows


def capacity(width, rows):
    return FIXED + row_bytes(width) * sum(min(240, width * min(BAND, rows - first)) for first in range(0, rows, BAND))


def search(rgb):
    """the palette index 16..255 of every pixel of uint8 [..., 3]: the least squared distance over the 240 entries, the first of the nearest"""
    p = np.asarray(rgb, dtype=np.int64)
    distance = ((p[..., None, :] - PALETTE) ** 2).sum(axis=-1)
    return (16 + np.argmin(distance, axis=-1)).astype(np.int64)  # argmin returns the first of equal minima


def per_cent(v):
    return (100 * int(v) + 127) // 255


def prologue(width, rows):
    text = HOME + DCS + b'"1;1;%05d;%05d' % (width, rows)
    for n in range(16, 256):
        r, g, b = PALETTE[n - 16]
        text += b"#%03d;2;%03d;%03d;%03d" % (n, per_cent(r), per_cent(g), per_cent(b))
    return text


def formatter_of_indices(index):
    """the text of a frame of palette indices [rows, width], as the description states it"""
    rows, width = index.shape
    text = [prologue(width, rows)]
    bands = range(0, rows, BAND)
    for first in bands:
        band = index[first:first + BAND]
        colours = sorted(set(int(n) for n in band.ravel()))
        for n in colours:
            six = sum((band[j] == n).astype(np.int64) << j for j in range(band.shape[0]))
            last = b"-" if n == colours[-1] and first != bands[-1] else b"$"
            text.append(b"#%03d" % n + bytes((63 + six).astype(np.uint8)) + b"$" * (pad(width) - 1) + last)
    return b"".join(text) + END


def formatter(rgb):
    return formatter_of_indices(search(rgb))


def every_colour_image():
    """40 x 6: each of the 240 palette colours once"""
    return PALETTE.astype(np.uint8).reshape(6, 40, 3)


def colours_per_band(index):
    return [len(set(int(n) for n in index[first:first + BAND].ravel())) for first in range(0, index.shape[0], BAND)]


def read(text):
    """the structural reader: int64 [rows, width] palette indices of a text, every rule of the format asserted on the way"""
    text = bytes(text)
    assert b"\n" not in text and b"\0" not in text
    assert text.startswith(HOME + DCS), text[:16]
    at = len(HOME) + len(DCS)
    raster = re.fullmatch(rb'"1;1;(\d{5});(\d{5})', text[at:at + 16])
    assert raster, text[at:at + 16]
    width, rows = int(raster.group(1)), int(raster.group(2))
    assert width > 0 and rows > 0
    at += 16
    for n in range(16, 256):
        r, g, b = PALETTE[n - 16]
        want = b"#%03d;2;%03d;%03d;%03d" % (n, per_cent(r), per_cent(g), per_cent(b))
        assert text[at:at + 18] == want, (n, text[at:at + 18], want)
        assert all(abs(per_cent(v) / 100 - v / 255) <= 0.005 + 1e-12 for v in (r, g, b))
        at += 18
    assert at == FIXED - 2
    assert text.endswith(END), text[-4:]
    body = text[at:-2]
    L, T = row_bytes(width), pad(width)
    assert len(body) % L == 0 and len(body) >= L, "the colour rows are not whole"
    index = np.zeros((rows, width), dtype=np.int64)
    bands = (rows + BAND - 1) // BAND
    band, previous = 0, 0
    for q in range(len(body) // L):
        row = body[q * L:(q + 1) * L]
        assert band < bands, "colour rows behind the last band"
        assert re.fullmatch(rb"#\d{3}", row[:4]), row[:4]
        n = int(row[1:4])
        assert 16 <= n <= 255 and n > previous, f"colour {n} behind {previous} in band {band}"
        data = np.frombuffer(row[4:4 + width], dtype=np.uint8).astype(np.int64)
        assert ((data >= 63) & (data <= 126)).all(), "a data character outside ?..~"
        six = data - 63
        assert six.any(), f"colour row {n} of band {band} paints no pixel"
        band_rows = min(BAND, rows - BAND * band)
        assert not (six >> band_rows).any(), f"a bit set in a row >= {rows}"
        for j in range(band_rows):
            here = ((six >> j) & 1).astype(bool)
            assert not (index[BAND * band + j][here] != 0).any(), f"a pixel of band {band} painted twice"
            index[BAND * band + j][here] = n
        assert row[4 + width:L - 1] == b"$" * (T - 1), row[4 + width:]
        closes = row[L - 1:L]
        assert closes in (b"$", b"-"), closes
        if closes == b"-":
            assert band + 1 < bands, "'-' behind the last band"
            band, previous = band + 1, 0
        else:
            previous = n
    assert band == bands - 1, f"the text ends in band {band} of {bands}"
    assert (index != 0).all(), "a pixel that no colour row paints"
    # a '-' stands behind the LAST colour of a band only: a band cut in two by one would leave a pixel of its rows unpainted or paint
    # the next band's rows, both of which have been refused above
    assert len(text) == length(width, len(body) // L)
    return index
