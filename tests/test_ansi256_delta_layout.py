"""The formats of the delta texts in the xterm 256-colour palette and the arithmetic the device kernels place their records by
(csrc/trt_ansi256_delta.h, csrc/trt_ansi256_delta_half.h), without a GPU: the headers the kernels compile are compiled for the host in
tests/ansi256_delta_check.c and tests/ansi256_delta_half_check.c -- programs of their own, which assemble the text by calling the kernels'
own lane walk for every tile and every thread (tests/ansi256_delta_check.h) over twenty-one families of frame pairs in two modes, hold it
against the sequential emitters (csrc/host/trt_emit.c), which use neither the headers nor the closed form of the palette map, and hold
the bounds against an enumeration of every row of 1..12 cells -- run plain and under the address and undefined-behaviour sanitizers.
Nothing is loaded into Python."""
import os
import subprocess

import pytest

import support as T

EMITTER = os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]
PROGRAMS = ["ansi256_delta_check", "ansi256_delta_half_check"]


def _build_and_run(program, name, flags):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    sources = [os.path.join(T.ROOT, "tests", program + ".c"), EMITTER]
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe] + sources, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("program", PROGRAMS)
def test_the_header_against_the_sequential_emitter(program):
    """text and length equal the emitter's, every byte stored once and none at or behind the length, nothing for bytes that move inside a
    palette entry, the bound reached by the "longest" family and equal to the longest of every row of 1..12 cells, the limits"""
    run = _build_and_run(program, program, ["-O2"])
    assert run.returncode == 0 and program + ": ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


@pytest.mark.parametrize("program", PROGRAMS)
def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(program):
    """the frames are allocated to the byte: a load behind a frame, or behind an odd half-block frame's last row, ends the program"""
    run = _build_and_run(program, program + "_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert run.returncode == 0 and program + ": ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
