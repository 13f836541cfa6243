"""The layout of a frame's DEC sixel image and the lane map of the device kernels that write it (csrc/trt_sixel.h), without a GPU: the
header the kernels compile is compiled for the host in tests/sixel_check.c -- a program of its own, which assembles the text through the
header's position map and lane map, band by band and thread by thread as the kernels go about it, at each of the four store alignments,
and holds it against the sequential emitter trt_emitter_sixel_rgb8 (csrc/host/trt_emit.c) -- and run plain and under the address and
undefined-behaviour sanitizers.  Nothing sanitized is loaded into Python.  The emitter itself is held against independent statements of the
format: a formatter written here from the format's description with a palette search of its own, a literal, and a structural reader that
stands in for a terminal (tests/sixel_support.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sixel_support as X
import support as T
from terminalraytracer_amd import hip, host

SOURCES = [os.path.join(T.ROOT, "tests", "sixel_check.c"), os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")]
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]
HOST_ARGUMENT = -106  # TRT_HOST_ERR_ARGUMENT (include/trt_host.h)
# (width, rows): the widths 1..5 have every T and colour rows shorter than a word or two; the rows 1, 5, 6, 7, 13 have a short only band, a
# whole one, a band of one row behind a whole one and two whole bands with one row left; 63, 64, 65 and 257 wide
SIZES = [(w, h) for w in (1, 2, 3, 4, 5) for h in (1, 5, 6, 7, 13)] + [(63, 7), (64, 6), (65, 13), (257, 5), (257, 13)]


def _build_and_run(name, flags):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe] + SOURCES, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=900)


def test_the_layout_header_and_the_lane_map_on_the_host():
    """the widths 1..9, 63..65, 255..258 and 1025 with the rows 1, 5, 6, 7, 13, 40 x 6 with every colour, 160 x 48 and 1 x 6151, pictures of
    few colours, one, every one and bands that alternate, at every address modulo the 4-byte store: the text assembled through the header's
    masks, scan, position map and lane map is the emitter's, every byte stored once and none outside, words at aligned addresses only"""
    run = _build_and_run("sixel_check", ["-O2"])
    assert run.returncode == 0 and "sixel_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers():
    run = _build_and_run("sixel_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert run.returncode == 0 and "sixel_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def _image(w, h, colours=None):
    """random bytes; with `colours`, that many random colours only"""
    rng = np.random.default_rng(1000 * w + h)
    if colours is None:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return rng.integers(0, 256, (colours, 3), dtype=np.uint8)[rng.integers(0, colours, (h, w))]


def _images(w, h):
    return [("random", _image(w, h)), ("five colours", _image(w, h, 5)), ("one colour", np.full((h, w, 3), (255, 0, 9), dtype=np.uint8))]


def test_the_formatters_search_is_the_librarys():
    rgb = np.random.default_rng(5).integers(0, 256, (4096, 3), dtype=np.uint8)
    lib = host.lib()
    assert [int(n) for n in X.search(rgb)] == [lib.trt_xterm256_index_search(int(r), int(g), int(b)) for r, g, b in rgb]
    assert np.array_equal(X.search(X.PALETTE.astype(np.uint8)), np.arange(16, 256))


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_the_emitter_against_a_formatter_written_from_the_format_and_the_reader(w, h):
    """byte for byte the formatter's text; the reader accepts it and returns the frame of palette indices; the length is the format's"""
    for name, image in _images(w, h):
        got = host.emitter_sixel_rgb8(image).tobytes()
        index = X.search(image)
        assert got == X.formatter(image), name
        assert len(got) == X.length(w, sum(X.colours_per_band(index))) <= X.capacity(w, h) == hip.sixel_capacity(w, h), name
        assert np.array_equal(X.read(got), index), name


def test_the_emitter_against_the_literal():
    one = np.array([[[255, 0, 9]]], dtype=np.uint8)
    got = host.emitter_sixel_rgb8(one).tobytes()
    assert len(got) == 4360 and got.endswith(b"#196@$$$\033\\")
    assert got.startswith(b'\033[0;0H\033P0;1;0q"1;1;00001;00001#016;2;000;000;000#017;2;000;000;037')
    assert b"#231;2;100;100;100#232;2;003;003;003#233;2;007;007;007" in got and b"#255;2;093;093;093#196@" in got


def test_every_colour_once_fills_the_capacity():
    image = X.every_colour_image()
    got = host.emitter_sixel_rgb8(image).tobytes()
    assert len(got) == 15872 == hip.sixel_capacity(40, 6) == X.capacity(40, 6)
    assert got == X.formatter(image)
    assert np.array_equal(X.read(got), np.arange(16, 256).reshape(6, 40))


def test_the_structural_reader_refuses_what_breaks_the_format():
    image = _image(9, 13, 5)  # three bands, T = 3, L = 16
    good = host.emitter_sixel_rgb8(image).tobytes()
    index = X.read(good)
    assert np.array_equal(index, X.search(image)) and X.colours_per_band(index)[0] >= 2
    L, first = X.row_bytes(9), X.FIXED - 2
    rows = [good[first + q * L:first + (q + 1) * L] for q in range((len(good) - X.FIXED) // L)]
    assert rows[0][-1:] == b"$" and b"".join(rows) == good[first:-2]
    swapped = good[:first] + rows[1] + rows[0] + b"".join(rows[2:]) + X.END                      # the colour order
    dashed = good[:first] + rows[0][:-1] + b"-" + b"".join(rows[1:]) + X.END                     # a "-" inside a band
    twice = good[:first] + rows[0] + rows[1][:4] + rows[0][4:4 + 9] + rows[1][4 + 9:] + b"".join(rows[2:]) + X.END  # colour 1 paints colour 0's pixels
    per_cent = good.replace(b"#017;2;000;000;037", b"#017;2;000;000;038")
    broken = [good[:100] + good[101:], good[:-1], good[1:], good + b"\0", swapped, dashed, twice, per_cent,
              good.replace(b"\033P0;1;0q", b"\033P0;0;0q"), good.replace(b'"1;1;00009', b'"1;1;00008'), good[:first] + b"".join(rows[1:]) + X.END]
    assert per_cent != good and twice != good and all(len(bad) > 0 for bad in broken)
    for k, bad in enumerate(broken):
        with pytest.raises((AssertionError, ValueError)):
            X.read(bad)
            pytest.fail(f"the reader accepted broken text {k}")
    text = host.emitter_sixel_rgb8(_image(3, 7, 2)).tobytes()  # rows 7: the second band has one row
    assert X.read(text).shape == (7, 3)
    at = len(text) - 2 - X.row_bytes(3) + 4
    with pytest.raises(AssertionError):  # a bit set in a row behind the last
        X.read(text[:at] + bytes([63 + ((text[at] - 63) | 2)]) + text[at + 1:])


@pytest.mark.parametrize("w,h", SIZES + [(40, 6), (160, 48), (480, 280), (1920, 1080)], ids=lambda v: str(v))
def test_sixel_capacity_is_the_formats_bound(w, h):
    assert hip.sixel_capacity(w, h) == X.capacity(w, h)


def test_sixel_capacity_of_known_sizes_of_no_screen_and_at_the_limits():
    assert hip.sixel_capacity(1, 1) == 4360 and hip.sixel_capacity(40, 6) == 15872 and hip.sixel_capacity(1920, 1080) == 4352 + 1928 * 240 * 180
    assert hip.sixel_capacity(2, 6) == 4352 + 8 * 12 and hip.sixel_capacity(1, 7) == 4352 + 8 * 7
    assert hip.sixel_capacity(0, 5) == hip.sixel_capacity(5, 0) == hip.sixel_capacity(-3, 4) == hip.sixel_capacity(4, -3) == 0
    assert hip.sixel_capacity(100000, 1) == hip.sixel_capacity(1, 100000) == 0
    assert hip.sixel_capacity(99999, 1) == X.capacity(99999, 1) and hip.sixel_capacity(99999, 99999) == 4352 + 100004 * 240 * 16667 > 1 << 32


def test_the_emitter_refuses_null_sizes_that_are_not_positive_or_above_the_limits_and_a_short_capacity():
    lib = host.lib()
    rgb = _image(7, 5, 4)
    want = X.formatter(rgb)
    need = len(want)
    assert need < X.capacity(7, 5)  # the text it would write, not the bound, is what the capacity must hold
    text = np.full(X.capacity(7, 5) + 8, 0xA5, dtype=np.uint8)
    n = C.c_size_t(12345)
    call = lambda src=rgb.ctypes.data, w=7, h=5, out=text.ctypes.data, cap=need, count=C.byref(n): lib.trt_emitter_sixel_rgb8(src, w, h, out, cap, count)
    assert call(src=None) == HOST_ARGUMENT and call(out=None) == HOST_ARGUMENT and call(count=None) == HOST_ARGUMENT
    assert call(w=0) == HOST_ARGUMENT and call(w=-7) == HOST_ARGUMENT and call(h=0) == HOST_ARGUMENT and call(h=-5) == HOST_ARGUMENT
    assert call(w=100000, cap=1 << 40) == HOST_ARGUMENT and call(h=100000, cap=1 << 40) == HOST_ARGUMENT
    assert call(cap=need - 1) == HOST_ARGUMENT and call(cap=0) == HOST_ARGUMENT
    assert (text == 0xA5).all() and n.value == 12345, "a refused call wrote"
    assert call() == 0 and n.value == need  # to the byte
    assert text[:need].tobytes() == want and (text[need:] == 0xA5).all()
    assert call(cap=X.capacity(7, 5)) == 0 and n.value == need and text[:need].tobytes() == want and (text[need:] == 0xA5).all()
