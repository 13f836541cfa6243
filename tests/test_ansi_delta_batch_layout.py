"""A chain of delta texts -- a shown frame, n frames back to back, text b between frames b - 1 and b, the n texts back to back as ONE prefix
sum over the tiles of n pairs of frames (csrc/trt_ansi_delta_chain.h) -- without a GPU: the headers the chain kernels compile are compiled
for the host in tests/ansi_delta_chain_check.c, a program of its own, once per kind of cell.  It assembles the texts the way the device
does -- the kind's own lane walk for every pair, tile and thread, one scan over all n * tiles sums in turns of TRT_DELTA_SCAN_BLOCK, the
lengths from the offsets -- and holds every text and length against the sequential emitters of csrc/host/trt_emit.c, with a store count per
byte; the n frames are one allocation to the byte.  Run plain and under the address and undefined-behaviour sanitizers.  Nothing is loaded
into Python."""
import os
import subprocess

import pytest

import support as T

SOURCES = [os.path.join(T.ROOT, "tests", "ansi_delta_chain_check.c"), os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")]
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]
KINDS = {"full": ("ansi_delta_chain_check", []), "half": ("ansi_delta_half_chain_check", ["-DCHAIN_HALF"])}
PLAIN = ["-O2"]
SANITIZED = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _build_and_run(name, flags):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe] + SOURCES, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("flags", [PLAIN, SANITIZED], ids=["plain", "sanitized"])
def test_the_chain_header_against_the_sequential_emitters(kind, flags):
    """n in {1, 2, 3, 8} frames of 1x1 to 160x47 whose steps cycle through equal frames, everything changed, 40 %, the frame before last, the
    first and the last cell, and n = 8 with more than 1024 tiles in all: texts, lengths and starts are the emitter's, every byte of the texts
    stored once and none outside them"""
    name, define = KINDS[kind]
    run = _build_and_run(name + ("_san" if flags is SANITIZED else ""), flags + define)
    assert run.returncode == 0 and name + ": ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
