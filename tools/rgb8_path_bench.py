"""What a host whose only consumer is the terminal emitter pays per frame: trt_render_host_rgb8 (host camera in, 3 bytes per pixel out) for
the demo scene at 480x280 and at 1920x1080, 10 bounces, 10 rays per pixel, and the share of it that the pass behind the render kernel
takes (reduce_ms of trt_render_kernel_times).  With --parent PATH the same calls go to a second build of the library in the same
process, the two taking turns round by round, so that the spread of one build over the rounds stands beside the difference between the
two.  For the build in the tree also: eight cameras per call at 1080p as bytes (trt_render_host_batch_rgb8) beside the same batch as
doubles (trt_render_host_batch).  Prints a markdown report (profiles/r08/a_rgb8.md is one)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S

B, SPP = 10, 10
SIZES = ((480, 280, 1000), (1920, 1080, 200))  # width, height, calls per round


def load(path):
    """the library at `path` with the prototypes of hip.SYMBOLS for every symbol it exports (an older build lacks the newer ones)"""
    try:
        import torch  # noqa: F401  (one HIP runtime per process, hip.lib())
    except ImportError:
        pass
    dll = C.CDLL(path)
    for name, (res, args) in hip.SYMBOLS.items():
        fn = getattr(dll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return dll


class Renderer:
    def __init__(self, label, dll, w, h):
        self.label, self.dll, self.w, self.h = label, dll, w, h
        self.ctx = C.c_void_p()
        self.check(dll.trt_create(0, C.byref(self.ctx)))
        self.scene = S.demo_scene(S.synth_sky(256), S.orbit_camera(1.0, w, h))
        self.keep = self.scene.as_scene()
        self.check(dll.trt_set_scene(self.ctx, C.byref(self.keep)))
        self.cam = hip.camera_struct(self.scene.camera)
        self.rows = hip.RowSet.whole(w, h)
        self.rgb = np.zeros((h, w, 3), dtype=np.uint8)

    def check(self, code):
        if code:
            raise RuntimeError(f"{self.label}: {self.dll.trt_last_error().decode()}")

    def call(self):
        self.check(self.dll.trt_render_host_rgb8(self.ctx, C.byref(self.cam), C.byref(self.rows), B, SPP, self.rgb.ctypes.data))

    def round(self, calls):
        """(host ms per call, median reduce_ms of the round's launches)"""
        t0 = time.perf_counter()
        for _ in range(calls):
            self.call()
        ms = (time.perf_counter() - t0) / calls * 1e3
        n = min(calls, 256)
        a, b = (C.c_float * n)(), (C.c_float * n)()
        got = self.dll.trt_render_kernel_times(self.ctx, a, b, n)
        return ms, statistics.median(b[:got])

    def close(self):
        self.dll.trt_destroy(self.ctx)


def spread(values):
    return f"{statistics.median(values):.4f} (min {min(values):.4f}, max {max(values):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a second build of libtrt_hip.so to measure in turn with the one in the tree")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    libs = [("this build", load(hip.LIB_PATH))]
    if args.parent:
        libs.insert(0, ("parent", load(args.parent)))
    print(f"# trt_render_host_rgb8, demo scene, {B} bounces, {SPP} rays per pixel\n")
    print(f"{args.rounds} rounds per size, the builds taking turns within a round; a cell is the median over the rounds (min, max).\n")
    print("| size | build | host ms per call | reduce_ms (the pass behind the render kernel) |")
    print("|---|---|---|---|")
    frames = {}
    for w, h, calls in SIZES:
        renderers = [Renderer(label, dll, w, h) for label, dll in libs]
        for r in renderers:
            for _ in range(20):
                r.call()
            frames[(w, h, r.label)] = r.rgb.copy()
        results = {r.label: ([], []) for r in renderers}
        for _ in range(args.rounds):
            for r in renderers:
                ms, reduce_ms = r.round(calls)
                results[r.label][0].append(ms)
                results[r.label][1].append(reduce_ms)
        for r in renderers:
            print(f"| {w}x{h} | {r.label} | {spread(results[r.label][0])} | {spread(results[r.label][1])} |")
            r.close()
        if args.parent:
            same = np.array_equal(frames[(w, h, "parent")], frames[(w, h, "this build")])
            print(f"| {w}x{h} | bytes of the two builds | {'identical' if same else 'DIFFERENT'} | |")
    # eight cameras per call at 1080p
    w, h, n = 1920, 1080, 8
    scene = S.demo_scene(S.synth_sky(256), S.orbit_camera(1.0, w, h))
    cams = np.stack([S.orbit_camera(1.0 + 0.05 * k, w, h) for k in range(n)])
    rows = hip.RowSet.whole(w, h)
    with hip.Context(0) as ctx:
        ctx.set_scene(scene)
        lib = hip.lib()
        out8, out64 = np.zeros((n, h, w, 3), dtype=np.uint8), np.zeros((n, h, w, 3), dtype=np.float64)  # the caller's buffers, reused like main()'s
        kinds = (("trt_render_host_batch_rgb8", out8), ("trt_render_host_batch", out64))
        run = lambda name, out: hip._check(getattr(lib, name)(ctx._h, cams.ctypes.data, n, C.byref(rows), B, SPP, out.ctypes.data))
        per = {name: [] for name, _ in kinds}
        for name, out in kinds:
            run(name, out)
        for _ in range(min(args.rounds, 5)):
            for name, out in kinds:
                t0 = time.perf_counter()
                for _ in range(4):
                    run(name, out)
                per[name].append((time.perf_counter() - t0) / (4 * n) * 1e3)
        print(f"\n# eight cameras per call, {w}x{h}, this build\n")
        print("| entry | host ms per frame |")
        print("|---|---|")
        for name, _ in kinds:
            print(f"| {name} | {spread(per[name])} |")

if __name__ == "__main__":
    main()
