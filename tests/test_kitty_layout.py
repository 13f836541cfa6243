"""The layout of a frame's kitty graphics-protocol image and the lane map of the device pass that writes it (csrc/trt_kitty.h), without a
GPU: the header the kernels compile is compiled for the host in tests/kitty_check.c -- a program of its own, which holds the text assembled
through the header's map, position by position and then wave by wave as the kernel goes about it, against the sequential emitter
trt_emitter_kitty_rgb8 (csrc/host/trt_emit.c) -- and run plain and under the address and undefined-behaviour sanitizers.  Nothing sanitized
is loaded into Python.  The emitter itself is held against independent statements of the format: a formatter written here from the
format's description around the standard library's base64, a literal, and a structural reader that stands in for a terminal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kitty_support as K
import support as T
from terminalraytracer_amd import hip, host

SOURCES = [os.path.join(T.ROOT, "tests", "kitty_check.c"), os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")]
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]
HOST_ARGUMENT = -106  # TRT_HOST_ERR_ARGUMENT (include/trt_host.h)
SIZES = [(1, 1), (1, 2), (3, 2), (7, 5), (21, 3), (8, 8), (13, 5), (341, 3), (32, 32), (41, 25), (683, 3), (67, 31)]  # (width, rows)


def _build_and_run(name, flags):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe] + SOURCES, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=900)


def test_the_layout_header_and_the_lane_map_on_the_host():
    """every P in 1..70, 1020..1030, 2044..2052 and 4095..4098 as every width x rows, 160 x 48, 480 x 280 and 1920 x 1080 against the emitter,
    every position classified once; the wave's lane map for batches of 1..3 frames at every address modulo the 4-byte store: every byte
    stored once, none outside, at most 65 pixels per wave, no pixel formed more than twice and at most one per wave a second time"""
    run = _build_and_run("kitty_check", ["-O2"])
    assert run.returncode == 0 and "kitty_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers():
    run = _build_and_run("kitty_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert run.returncode == 0 and "kitty_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def _image(w, h):
    return K.every_value_image() if (w, h) == (16, 16) else np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("w,h", SIZES + [(16, 16)], ids=lambda v: str(v))
def test_the_emitter_against_a_formatter_written_from_the_format(w, h):
    image = _image(w, h)
    got = host.emitter_kitty_rgb8(image).tobytes()
    assert len(got) == K.length(w, h)
    assert got == K.formatter(image)


def test_the_emitter_against_the_literal():
    one = np.array([[[255, 0, 9]]], dtype=np.uint8)
    assert host.emitter_kitty_rgb8(one).tobytes() == b"\033[0;0H\033_Ga=T,f=24,i=1,p=1,q=2,C=1,s=00001,v=00001,m=0;/wAJ\033\\"


@pytest.mark.parametrize("w,h", SIZES + [(16, 16), (160, 48)], ids=lambda v: str(v))
def test_the_structural_reader_reads_the_emitters_text_back_to_the_frame(w, h):
    """the prefix, the first sequence's keys, `m` alone in every later one, payloads of at most 4096 characters and a multiple of 4, m=1
    everywhere but last, and the joined payload decodes -- strictly -- to exactly the frame"""
    image = _image(w, h)
    assert np.array_equal(K.read(host.emitter_kitty_rgb8(image)), image)


def test_the_structural_reader_refuses_what_breaks_the_format():
    image = _image(41, 25)  # 1025 pixels: two chunks
    good = host.emitter_kitty_rgb8(image).tobytes()
    assert np.array_equal(K.read(good), image)
    first_m = good.index(b"m=1;")
    for bad in (good[1:], good + b"\0", good[:-2], good.replace(b"a=T", b"a=t"), good[:first_m] + b"m=0;" + good[first_m + 4:],
                good.replace(b"\033_Gm=00;", b"\033_Gq=2,m=0;"), good[:60] + b"=" + good[61:]):
        with pytest.raises((AssertionError, ValueError)):
            K.read(bad)


@pytest.mark.parametrize("w,h", SIZES + [(16, 16), (160, 48), (480, 280), (1920, 1080)], ids=lambda v: str(v))
def test_kitty_bytes_is_the_formats_length(w, h):
    assert hip.kitty_bytes(w, h) == K.length(w, h)


def test_kitty_bytes_of_known_sizes_of_no_screen_and_above_the_limits():
    assert hip.kitty_bytes(1, 1) == 60 and hip.kitty_bytes(160, 48) == 30846 and hip.kitty_bytes(480, 280) == 538966 and hip.kitty_bytes(1920, 1080) == 8314696
    assert hip.kitty_bytes(0, 5) == hip.kitty_bytes(5, 0) == hip.kitty_bytes(-3, 4) == hip.kitty_bytes(4, -3) == 0
    assert hip.kitty_bytes(100000, 1) == hip.kitty_bytes(1, 100000) == 0
    assert hip.kitty_bytes(99999, 1) == K.length(99999, 1) and hip.kitty_bytes(99999, 99999) == K.length(99999, 99999) > 1 << 32


def test_the_emitter_refuses_null_sizes_that_are_not_positive_or_above_the_limits_and_a_short_capacity():
    lib = host.lib()
    rgb = np.random.default_rng(3).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    need = K.length(7, 5)
    text = np.full(need + 8, 0xA5, dtype=np.uint8)
    n = C.c_size_t(12345)
    call = lambda src=rgb.ctypes.data, w=7, h=5, out=text.ctypes.data, cap=need, count=C.byref(n): lib.trt_emitter_kitty_rgb8(src, w, h, out, cap, count)
    assert call(src=None) == HOST_ARGUMENT and call(out=None) == HOST_ARGUMENT and call(count=None) == HOST_ARGUMENT
    assert call(w=0) == HOST_ARGUMENT and call(w=-7) == HOST_ARGUMENT and call(h=0) == HOST_ARGUMENT and call(h=-5) == HOST_ARGUMENT
    assert call(w=100000, cap=1 << 40) == HOST_ARGUMENT and call(h=100000, cap=1 << 40) == HOST_ARGUMENT
    assert call(cap=need - 1) == HOST_ARGUMENT and call(cap=0) == HOST_ARGUMENT
    assert (text == 0xA5).all() and n.value == 12345, "a refused call wrote"
    assert call() == 0 and n.value == need  # to the byte
    assert text[:need].tobytes() == K.formatter(rgb) and (text[need:] == 0xA5).all()
