"""The layout of a frame's half-block terminal text and the lane map of the device pass that writes it (csrc/trt_ansi_half.h), without a
GPU: the header the kernels compile is compiled for the host in tests/ansi_half_check.c -- a program of its own, which holds the text
assembled through the header's map, position by position and then wave by wave as the kernel goes about it, against the sequential
emitter trt_emitter_half_rgb8 (csrc/host/trt_emit.c) -- and run plain and under the address and undefined-behaviour sanitizers.  Nothing
sanitized is loaded into Python.  The emitter itself is held against two independent statements of the format: a formatter written
here from the format's description, and literals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import support as T
from terminalraytracer_amd import hip, host

SOURCES = [os.path.join(T.ROOT, "tests", "ansi_half_check.c"), os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")]
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]
HOST_ARGUMENT = -106  # TRT_HOST_ERR_ARGUMENT (include/trt_host.h)
SIZES = [(1, 1), (1, 2), (2, 3), (3, 2), (4, 4), (7, 5), (67, 13)]  # (width, rows)


def _build_and_run(name, flags):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe] + SOURCES, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=900)


def test_the_layout_header_and_the_lane_map_on_the_host():
    """every width 1..70 x rows 1..5, 160 x 48, 480 x 280 and 1920 x 1080 against the emitter, every position classified once, advance and step
    against locate at every byte; the wave's lane map for batches of 1..3 frames at every address modulo the 4-byte store: every byte stored
    once, none outside, at most 64 cells per wave, the head in the prefix and the tail in the last 5 bytes"""
    run = _build_and_run("ansi_half_check", ["-O2"])
    assert run.returncode == 0 and "ansi_half_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers():
    run = _build_and_run("ansi_half_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert run.returncode == 0 and "ansi_half_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def formatter(rgb):
    """the format as its description states it, in format strings: the home prefix; per pair of rows a cell per column -- foreground the upper
    row's pixel, background the lower row's (black behind an odd frame's last row), the glyph U+2580 -- and a reset and a newline"""
    rows, width, _ = rgb.shape
    text = "\033[0;0H"
    for top in range(0, rows, 2):
        for col in range(width):
            fg = rgb[top, col]
            bg = rgb[top + 1, col] if top + 1 < rows else (0, 0, 0)
            text += "\033[38;2;%03d;%03d;%03d;48;2;%03d;%03d;%03dm▀" % (*fg, *bg)
        text += "\033[0m\n"
    return text.encode("utf-8")


def every_value_image():
    i = np.arange(256)
    image = np.stack([i, 255 - i, (7 * i) & 255], axis=1).astype(np.uint8).reshape(16, 16, 3)
    assert all(len(set(image[..., ch].ravel())) == 256 for ch in range(3))
    return image


@pytest.mark.parametrize("w,h", SIZES + [(16, 16)], ids=lambda v: str(v))
def test_the_emitter_against_a_formatter_written_from_the_format(w, h):
    image = every_value_image() if (w, h) == (16, 16) else np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = host.emitter_half_rgb8(image).tobytes()
    assert len(got) == 6 + (39 * w + 5) * ((h + 1) // 2)
    assert got == formatter(image)


def test_the_emitter_against_literals():
    """which half is which, and what an odd frame's lower half is"""
    two = np.array([[[1, 2, 3]], [[4, 5, 6]]], dtype=np.uint8)  # width 1, rows 2: upper (1,2,3), lower (4,5,6)
    assert host.emitter_half_rgb8(two).tobytes() == b"\033[0;0H\033[38;2;001;002;003;48;2;004;005;006m\xe2\x96\x80\033[0m\n"
    one = np.array([[[255, 0, 9]]], dtype=np.uint8)
    assert host.emitter_half_rgb8(one).tobytes() == b"\033[0;0H\033[38;2;255;000;009;48;2;000;000;000m\xe2\x96\x80\033[0m\n"


@pytest.mark.parametrize("w,h", SIZES + [(16, 16), (160, 48), (480, 280), (1920, 1080)], ids=lambda v: str(v))
def test_ansi_half_bytes_is_the_formats_length(w, h):
    assert hip.ansi_half_bytes(w, h) == 6 + (39 * w + 5) * ((h + 1) // 2)


def test_ansi_half_bytes_of_known_sizes_and_of_no_screen():
    assert hip.ansi_half_bytes(160, 48) == 149886 and hip.ansi_half_bytes(480, 280) == 2621506 and hip.ansi_half_bytes(66, 5) == 7743
    assert hip.ansi_half_bytes(0, 5) == hip.ansi_half_bytes(5, 0) == hip.ansi_half_bytes(-3, 4) == hip.ansi_half_bytes(4, -3) == 0
    assert hip.ansi_half_bytes(85899346, 5) == 6 + (39 * 85899346 + 5) * 3 > 1 << 32  # beyond 2^32 bytes
    assert hip.ANSI_HALF_WAVE_WORDS % 64 == 0 and (38 + 4 * hip.ANSI_HALF_WAVE_WORDS - 1) // 39 + 1 <= 64


def test_the_emitter_refuses_null_sizes_that_are_not_positive_and_a_short_capacity():
    lib = host.lib()
    rgb = np.random.default_rng(3).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    need = 6 + (39 * 7 + 5) * 3
    text = np.full(need + 8, 0xA5, dtype=np.uint8)
    n = C.c_size_t(12345)
    call = lambda src=rgb.ctypes.data, w=7, h=5, out=text.ctypes.data, cap=need, count=C.byref(n): lib.trt_emitter_half_rgb8(src, w, h, out, cap, count)
    assert call(src=None) == HOST_ARGUMENT and call(out=None) == HOST_ARGUMENT and call(count=None) == HOST_ARGUMENT
    assert call(w=0) == HOST_ARGUMENT and call(w=-7) == HOST_ARGUMENT and call(h=0) == HOST_ARGUMENT and call(h=-5) == HOST_ARGUMENT
    assert call(cap=need - 1) == HOST_ARGUMENT and call(cap=0) == HOST_ARGUMENT
    assert (text == 0xA5).all() and n.value == 12345, "a refused call wrote"
    assert call() == 0 and n.value == need  # to the byte
    assert text[:need].tobytes() == formatter(rgb) and (text[need:] == 0xA5).all()
