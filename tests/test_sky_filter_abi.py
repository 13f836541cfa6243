"""The sky filter at the C boundary, without a device: the three entries and the two modes are declared in include/trt_hip.h, exported by
the library, bound by terminalraytracer_amd/hip.py with the same shapes, and examples/trt_demo takes --sky-filter."""
import ctypes as C
import os
import re
import subprocess

import support as T
from terminalraytracer_amd import hip

DECLARED = {"trt_set_sky_filter": "int trt_set_sky_filter(trt_context *ctx, int mode);",
            "trt_get_sky_filter": "int trt_get_sky_filter(trt_context *ctx, int *mode);",
            "trt_set_default_sky_filter": "int trt_set_default_sky_filter(int mode);"}
BOUND = {"trt_set_sky_filter": (C.c_int, [C.c_void_p, C.c_int]),
         "trt_get_sky_filter": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
         "trt_set_default_sky_filter": (C.c_int, [C.c_int])}


def header():
    with open(os.path.join(T.ROOT, "include", "trt_hip.h")) as fh:
        return fh.read()


def test_the_three_entries_are_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", header())
    dll = hip.lib()
    for name, declaration in DECLARED.items():
        assert declaration in text, name
        assert hasattr(dll, name), (name, "is not exported")
        assert hip.SYMBOLS[name] == BOUND[name], (name, hip.SYMBOLS[name])
    assert "#define TRT_SKY_NEAREST 0" in text and "#define TRT_SKY_BILINEAR 1" in text
    assert (hip.SKY_NEAREST, hip.SKY_BILINEAR) == (0, 1)
    assert callable(hip.Context.set_sky_filter) and callable(hip.Context.sky_filter) and callable(hip.set_default_sky_filter)


def test_the_header_declares_the_rules():
    text = re.sub(r"[\s*]+", " ", header())
    block = text[text.index("EXTENSION, PARITY UNPINNED. Bilinear filtering of the sky"):text.index("int trt_set_sky_filter(")]
    for phrase in ("U = (u + 0.5) dim", "x = clamp(U - 0.5, 0.0, dim - 1.0)", "i1 = (i0 + 1 < dim) ? i0 + 1 : i0", "top = t00 + (t10 - t00) fx",
                   "c = (top + (bot - top) fy) / 255.0", "face 0, all four taps texel 0 and fx = fy = 0", "TRT_SKY_FILTER=0|1", "TRT_ERR_CAPACITY"):
        assert phrase in block, phrase


def test_the_arguments_are_checked_without_a_device():
    """what needs no context: the default switch takes the two modes alone, and a NULL context is an argument error"""
    dll = hip.lib()
    try:
        assert dll.trt_set_default_sky_filter(2) == -2 and dll.trt_set_default_sky_filter(-1) == -2
        assert b"sky filter" in dll.trt_last_error()
        assert dll.trt_set_default_sky_filter(1) == 0 and dll.trt_set_default_sky_filter(0) == 0
        mode = C.c_int(7)
        assert dll.trt_set_sky_filter(None, 1) == -2 and b"ctx is NULL" in dll.trt_last_error(), "the context is at fault, not the 1"
        assert dll.trt_get_sky_filter(None, C.byref(mode)) == -2 and mode.value == 7
    finally:
        dll.trt_shutdown()  # forgets the default switch; there is no default context to destroy


def test_the_demo_takes_the_flag():
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    usage = subprocess.run([exe], capture_output=True, timeout=60)
    assert usage.returncode == 2 and b"[--sky-filter]" in usage.stderr
    # the flag is taken before anything touches a device or a file: with it the program gets as far as the skybox, which is not there
    for flags in (["--sky-filter"], ["--sky-filter", "--rgb8"], ["--sixel", "--sky-filter"], ["--half", "--delta", "--sky-filter", "--step=0.04", "--batch=2"]):
        run = subprocess.run([exe, os.path.join(T.ROOT, "no such skybox"), "1", "16", "8"] + flags, capture_output=True, timeout=60)
        assert run.returncode == 1 and b"cannot load skybox" in run.stderr and b"trt_set_default_sky_filter" not in run.stderr, (flags, run.stderr[-300:])
    clash = subprocess.run([exe, os.path.join(T.ROOT, "no such skybox"), "1", "16", "8", "--sky-filter", "--specular"], capture_output=True, timeout=60)
    assert clash.returncode == 2 and b"do not combine" in clash.stderr
