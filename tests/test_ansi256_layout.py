"""The layouts of the two terminal texts in the xterm 256-colour palette and the lane maps of the device pass that writes them
(csrc/trt_ansi256.h, csrc/trt_ansi256_half.h over csrc/trt_text_map.h), without a GPU: the headers the kernels compile are compiled for the
host in tests/ansi256_check.c and tests/ansi256_half_check.c -- programs of their own, which hold the text assembled through the headers'
maps, position by position and then wave by wave as the kernel goes about it, against the sequential emitters -- and run plain and under
the address and undefined-behaviour sanitizers.  Nothing sanitized is loaded into Python.  The emitters themselves are read back by a
reader written from the formats' description (tests/ansi256_support.py) and held against literals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ansi256_support as A
import support as T
from terminalraytracer_amd import hip, host

EMIT = os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
HOST_ARGUMENT = -106  # TRT_HOST_ERR_ARGUMENT (include/trt_host.h)
SIZES = [(1, 1), (1, 2), (2, 3), (3, 2), (5, 5), (40, 3), (67, 13), (67, 12), (130, 1)]  # (width, rows)
KINDS = pytest.mark.parametrize("half", [False, True], ids=["full", "half_block"])


def _build_and_run(program, name, flags):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe, os.path.join(T.ROOT, "tests", program + ".c"), EMIT],
                          capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize("program", ["ansi256_check", "ansi256_half_check"])
def test_the_layout_header_and_the_lane_map_on_the_host(program):
    """every width 1..70 x rows 1..3, the widths 40, 55..61, 63, 64, 65, 67 and 130 x rows 1, 2, 3 and 13, 160 x 48 and 480 x 280: every
    position's byte is the emitter's and is classified once; every word of every wave is claimed by exactly one lane, for batches of 1..3
    frames at every address modulo the 4-byte store; the lone bytes; at most 60 and 57 cells per span; the lengths of no screen"""
    run = _build_and_run(program, program, ["-O2"])
    assert run.returncode == 0 and program + ": ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


@pytest.mark.parametrize("program", ["ansi256_check", "ansi256_half_check"])
def test_the_same_programs_under_address_and_undefined_behaviour_sanitizers(program):
    run = _build_and_run(program, program + "_san", SANITIZE)
    assert run.returncode == 0 and program + ": ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def _image(w, h):
    return A.edge_frame(w, h, 7) if (w + h) % 2 else np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)


@KINDS
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_the_reader_reads_the_emitters_text_back_to_the_searchs_indices(w, h, half):
    """prefix, cells, row ends and nothing else; per cell the index trt_xterm256_index_search finds for the pixel; 016 below the last row of
    an odd half-block frame; the length is the formula's and trt_ansi256[_half]_bytes'"""
    image = _image(w, h)
    text = host.emitter_ansi256_rgb8(image, half)
    assert text.size == A.length(w, h, half) == hip.ansi256_bytes(w, h, half)
    shown = A.read(text, half)
    assert shown.shape[:2] == ((h + 1) // 2 if half else h, w)
    indices, below = A.frame_indices(shown, h, half)
    assert np.array_equal(indices, A.search(image))
    assert indices.min() >= 16 and indices.max() <= 255
    if half and h % 2:
        assert (below == 16).all() and text[-(23 * w + 5):].tobytes().count(b";48;5;016m") >= w
    else:
        assert below is None


def test_the_emitters_against_literals():
    one = np.array([[[255, 0, 9]]], dtype=np.uint8)  # nearest: (255, 0, 0), 16 + 180
    assert host.emitter_ansi256_rgb8(one).tobytes() == b"\033[0;0H\033[48;5;196m  \033[0m\n"
    assert host.emitter_ansi256_rgb8(one, half=True).tobytes() == b"\033[0;0H\033[38;5;196;48;5;016m\xe2\x96\x80\033[0m\n"
    two = np.array([[[128, 128, 128]], [[0, 0, 95]]], dtype=np.uint8)
    assert host.emitter_ansi256_rgb8(two).tobytes() == b"\033[0;0H\033[48;5;244m  \033[0m\n\033[48;5;017m  \033[0m\n"
    assert host.emitter_ansi256_rgb8(two, half=True).tobytes() == b"\033[0;0H\033[38;5;244;48;5;017m\xe2\x96\x80\033[0m\n"


@KINDS
def test_the_reader_refuses_what_breaks_the_format(half):
    good = host.emitter_ansi256_rgb8(_image(5, 3), half).tobytes()
    A.read(good, half)
    at = good.index(b"5;") + 2  # the first index's first digit
    for bad in (good[1:], good + b"\0", good[:-1], good[:at] + b" " + good[at + 1:], good.replace(b"\033[0m\n", b"\033[0m", 1), good.replace(b";5;", b";2;", 1)):
        with pytest.raises(AssertionError):
            A.read(bad, half)
    with pytest.raises(AssertionError):
        A.read(good, not half)


@KINDS
def test_the_lengths_of_known_sizes_and_of_no_screen(half):
    n = lambda w, h: hip.ansi256_bytes(w, h, half)
    assert n(0, 5) == n(5, 0) == n(-3, 4) == n(4, -3) == n(0, 0) == n(-1, -1) == 0
    assert n(1, 1) == (34 if half else 24) and n(160, 48) == (6 + 3685 * 24 if half else 6 + 2085 * 48)
    assert n(1920, 1080) == (6 + (23 * 1920 + 5) * 540 if half else 6 + (13 * 1920 + 5) * 1080)
    assert n(67, 13) == A.length(67, 13, half) and n(67, 12) == A.length(67, 12, half)
    assert hip.ansi256_bytes(67, 13, True) == hip.ansi256_bytes(67, 14, True)  # an odd frame has the text rows of the next even one


@KINDS
def test_the_emitters_refuse_null_sizes_that_are_not_positive_and_a_short_capacity(half):
    lib = host.lib()
    entry = lib.trt_emitter_ansi256_half_rgb8 if half else lib.trt_emitter_ansi256_rgb8
    rgb = np.random.default_rng(3).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    need = A.length(7, 5, half)
    text = np.full(need + 8, 0xA5, dtype=np.uint8)
    n = C.c_size_t(12345)
    call = lambda src=rgb.ctypes.data, w=7, h=5, out=text.ctypes.data, cap=need, count=C.byref(n): entry(src, w, h, out, cap, count)
    assert call(src=None) == HOST_ARGUMENT and call(out=None) == HOST_ARGUMENT and call(count=None) == HOST_ARGUMENT
    assert call(w=0) == HOST_ARGUMENT and call(w=-7) == HOST_ARGUMENT and call(h=0) == HOST_ARGUMENT and call(h=-5) == HOST_ARGUMENT
    assert call(cap=need - 1) == HOST_ARGUMENT and call(cap=0) == HOST_ARGUMENT
    assert (text == 0xA5).all() and n.value == 12345, "a refused call wrote"
    assert call() == 0 and n.value == need  # to the byte
    assert np.array_equal(text[:need], host.emitter_ansi256_rgb8(rgb, half)) and (text[need:] == 0xA5).all()
