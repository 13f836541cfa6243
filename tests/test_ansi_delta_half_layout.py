"""The format of the delta text in half-block cells and the arithmetic the device kernels place its records by
(csrc/trt_ansi_delta_half.h), without a GPU: the header the kernels compile is compiled for the host in tests/ansi_delta_half_check.c -- a
program of its own, which assembles the text by calling the kernels' own lane walk (trt_delta_half_lane_cells, trt_delta_half_lane_byte)
for every tile and every thread (the lanes' totals summed per tile, the exclusive scan of the tiles, each lane behind the lanes before
it; tests/ansi_delta_check.h) for every width 1..70 x rows 1..5, 160 x 47, 160 x 48 and
480 x 280 over eighteen families of frame pairs, and holds it against the sequential emitter trt_emitter_delta_half_rgb8
(csrc/host/trt_emit.c), which does not use the header -- run plain and under the address and undefined-behaviour sanitizers.  The frames
are allocated to the byte, so a read behind an odd frame's last row is the sanitizer's to report.  Nothing is loaded into Python."""
import os
import subprocess

import support as T

SOURCES = [os.path.join(T.ROOT, "tests", "ansi_delta_half_check.c"), os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")]
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]


def _build_and_run(name, flags):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe] + SOURCES, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def test_the_half_block_delta_header_against_the_sequential_emitter():
    """text and length equal the emitter's, every byte stored once and none at or behind the length, the bound reached where every cell
    changed and both colours differ from the left neighbour's, every record length seen, the limits and the size pins"""
    run = _build_and_run("ansi_delta_half_check", ["-O2"])
    assert run.returncode == 0 and "ansi_delta_half_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers():
    run = _build_and_run("ansi_delta_half_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert run.returncode == 0 and "ansi_delta_half_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
