"""The layout of a frame's terminal text and the lane map of the device pass that writes it (csrc/trt_ansi.h), without a GPU: the header
the kernels compile is compiled for the host in tests/ansi_check.c -- a program of its own, which holds the text assembled through the
header's map, position by position and then wave by wave as the kernel goes about it, against the host emitter's buffer
(csrc/host/trt_emit.c) -- and run plain and under the address and undefined-behaviour sanitizers.  Nothing is loaded into Python but
the library's own trt_ansi_bytes."""
import os
import subprocess

import pytest

import support as T
from terminalraytracer_amd import hip, host

SOURCES = [os.path.join(T.ROOT, "tests", "ansi_check.c"), os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")]
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]


def _build_and_run(name, flags):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe] + SOURCES, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def test_the_layout_header_and_the_lane_map_on_the_host():
    """every width 1..70 x rows 1..4 and a few larger screens against the emitter, every position classified once; the wave's lane map
    for batches of 1..3 frames at every address modulo the 4-byte store: every byte stored once, none outside"""
    run = _build_and_run("ansi_check", ["-O2"])
    assert run.returncode == 0 and "ansi_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers():
    run = _build_and_run("ansi_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert run.returncode == 0 and "ansi_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (7, 5), (67, 13), (160, 48), (480, 280), (1920, 1080)])
def test_ansi_bytes_is_the_emitters_size(w, h):
    e = host.Emitter(w, h)
    try:
        assert hip.ansi_bytes(w, h) == 8 + (25 * w + 1) * h + 1 == len(e.bytes())
    finally:
        e.close()


def test_ansi_bytes_of_the_goldens_and_of_no_screen():
    for meta in T.golden_meta()["emitter"].values():
        assert hip.ansi_bytes(meta["width"], meta["height"]) == meta["bytes"]
    assert hip.ansi_bytes(0, 5) == hip.ansi_bytes(5, 0) == hip.ansi_bytes(-3, 4) == hip.ansi_bytes(4, -3) == 0
    assert hip.ansi_bytes(85899346, 25) == 9 + (25 * 85899346 + 1) * 25  # beyond 2^32 bytes
