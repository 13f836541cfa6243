"""The xterm 256-colour palette map without a GPU: csrc/trt_xterm256.h, the closed form the device kernels compute, is compiled for the host
in tests/xterm256_check.c -- a program of its own -- and held there against the rule itself, trt_xterm256_index_search's loop over the 240
fixed entries, on all 2^24 colours; the same program runs under the address and undefined-behaviour sanitizers on every 251st colour.
Nothing sanitized is loaded into Python.  The library's exported statements are held against the known answers and a search written here."""
import os
import subprocess

import numpy as np

import support as T
from terminalraytracer_amd import host

SOURCES = [os.path.join(T.ROOT, "tests", "xterm256_check.c"), os.path.join(T.ROOT, "terminalraytracer_amd", "csrc", "host", "trt_emit.c")]
INCLUDES = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")]
KNOWN = [((0, 0, 0), 16), ((255, 255, 255), 231), ((128, 128, 128), 244), ((115, 115, 115), 243), ((47, 48, 115), 238), ((4, 4, 4), 16),
         ((5, 5, 5), 232), ((13, 13, 13), 232), ((246, 246, 246), 255), ((247, 247, 247), 231)]
LEVELS = (0, 95, 135, 175, 215, 255)


def _build_and_run(name, flags, arguments=()):
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    made = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + ["-o", exe] + SOURCES, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    return subprocess.run([exe, *arguments], capture_output=True, text=True, timeout=900)


def test_the_closed_form_is_the_search_on_every_colour():
    """all 2^24 colours: the closed form equals the 240-entry search with the lowest index on ties; the known answers; every index 16..255
    occurs and none below 16"""
    run = _build_and_run("xterm256_check", ["-O2"])
    assert run.returncode == 0 and "xterm256_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers():
    run = _build_and_run("xterm256_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"], ["251"])
    assert run.returncode == 0 and "xterm256_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


def test_the_known_answers_through_the_library():
    for colour, index in KNOWN:
        assert host.xterm256_index(*colour) == index, colour
        assert host.xterm256_index_search(*colour) == index, colour


def _palette():
    cube = [(LEVELS[i], LEVELS[j], LEVELS[k]) for i in range(6) for j in range(6) for k in range(6)]
    return np.array(cube + [(8 + 10 * k,) * 3 for k in range(24)], dtype=np.int64)


def test_the_library_against_a_search_written_here():
    """4096 random colours, every grey and every palette entry itself: numpy's argmin returns the FIRST of the least, which is the rule"""
    palette = _palette()
    assert palette.shape == (240, 3)
    rng = np.random.default_rng(256)
    colours = np.concatenate([rng.integers(0, 256, (4096, 3)), np.repeat(np.arange(256), 3).reshape(256, 3), palette])
    want = 16 + np.argmin(((colours[:, None, :] - palette[None, :, :]) ** 2).sum(axis=2), axis=1)
    for colour, index in zip(colours, want):
        r, g, b = (int(v) for v in colour)
        assert host.xterm256_index_search(r, g, b) == index, (r, g, b)
        assert host.xterm256_index(r, g, b) == index, (r, g, b)
    for k, entry in enumerate(palette):
        assert host.xterm256_index(*(int(v) for v in entry)) == 16 + k  # an entry is its own nearest
