"""What a host whose only consumer is the terminal pays per frame for the HALF-BLOCK text it writes, by two routes, for the demo scene at
480x280 and at 1920x1080, 10 bounces, 10 rays per pixel:

  (a) trt_render_host_rgb8 (3 bytes per pixel across PCIe) and trt_emitter_half_rgb8 (the digits formatted in a loop on the host);
  (b) trt_render_host_ansi_half (the text formatted by the pass behind the render kernel, 19.5 bytes per pixel across PCIe, nothing left to do).

A third route, trt_render_host_ansi (the full text, 25 bytes per pixel), runs beside them for its pass's reduce_ms at the same frame size in
the same process.  The routes take turns round by round, so that the spread of one route over the rounds stands beside the difference
between two.  Reported with the spread: host ms per frame of either route (of (a) also its two halves), reduce_ms (trt_render_kernel_times)
of the bytes pass, of the full-text pass and of the half-block pass, and whether (a)'s text and (b)'s are identical.  Prints a markdown
report (profiles/r13/a_half.md holds one)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import scenes as S

B, SPP = 10, 10
SIZES = ((480, 280, 400), (1920, 1080, 60))  # width, height, calls per round


def spread(values):
    return f"{statistics.median(values):.4f} (min {min(values):.4f}, max {max(values):.4f})"


class Routes:
    def __init__(self, w, h):
        self.w, self.h = w, h
        self.lib, self.hostlib = hip.lib(), host.lib()
        self.ctx = hip.Context(0)
        self.scene = S.demo_scene(S.synth_sky(256), S.orbit_camera(1.0, w, h))
        self.ctx.set_scene(self.scene)
        self.cam = hip.camera_struct(self.scene.camera)
        self.rows = hip.RowSet.whole(w, h)
        self.rgb = np.zeros((h, w, 3), dtype=np.uint8)  # the caller's buffers, reused like main()'s
        self.half = np.zeros(hip.ansi_half_bytes(w, h), dtype=np.uint8)
        self.half_on_host = np.zeros(hip.ansi_half_bytes(w, h), dtype=np.uint8)
        self.full = np.zeros(hip.ansi_bytes(w, h), dtype=np.uint8)

    def reduce_ms(self, calls):
        n = min(calls, 256)
        a, b = (C.c_float * n)(), (C.c_float * n)()
        got = self.lib.trt_render_kernel_times(self.ctx._h, a, b, n)
        return statistics.median(b[:got])

    def bytes_then_emitter(self, calls):
        """(host ms per frame, of which the render call, of which the emitter, reduce_ms of the bytes pass)"""
        render = emit = 0.0
        n = C.c_size_t(0)
        for _ in range(calls):
            t0 = time.perf_counter()
            hip._check(self.lib.trt_render_host_rgb8(self.ctx._h, C.byref(self.cam), C.byref(self.rows), B, SPP, self.rgb.ctypes.data))
            t1 = time.perf_counter()
            self.hostlib.trt_emitter_half_rgb8(self.rgb.ctypes.data, self.w, self.h, self.half_on_host.ctypes.data, self.half_on_host.size, C.byref(n))
            emit += time.perf_counter() - t1
            render += t1 - t0
        return (render + emit) / calls * 1e3, render / calls * 1e3, emit / calls * 1e3, self.reduce_ms(calls)

    def text_from_device(self, entry, out, calls):
        """(host ms per frame, reduce_ms)"""
        t0 = time.perf_counter()
        for _ in range(calls):
            hip._check(entry(self.ctx._h, C.byref(self.cam), C.byref(self.rows), B, SPP, out.ctypes.data))
        return (time.perf_counter() - t0) / calls * 1e3, self.reduce_ms(calls)

    def close(self):
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls-divisor", type=int, default=1, help="divide the calls per round (a shorter run)")
    args = ap.parse_args()
    print(f"# the terminal's half-block text of a frame by two routes, demo scene, {B} bounces, {SPP} rays per pixel\n")
    print("(a) trt_render_host_rgb8 + trt_emitter_half_rgb8; (b) trt_render_host_ansi_half; beside them trt_render_host_ansi for its pass.  "
          f"{args.rounds} rounds per size, the routes taking turns within a round; a cell is the median over the rounds (min, max), in ms.\n")
    print("| size | half-block text bytes | full text bytes | (a) host ms per frame | (a) render call | (a) emitter on the host | (b) host ms per frame | full text, host ms per frame | (a)'s text and (b)'s |")
    print("|---|---|---|---|---|---|---|---|---|")
    passes, verdicts = [], []
    for w, h, calls in SIZES:
        calls = max(calls // args.calls_divisor, 4)
        r = Routes(w, h)
        for _ in range(10):
            r.bytes_then_emitter(1)
            r.text_from_device(r.lib.trt_render_host_ansi_half, r.half, 1)
            r.text_from_device(r.lib.trt_render_host_ansi, r.full, 1)
        same = r.half_on_host.tobytes() == r.half.tobytes()
        a, b, full = [], [], []
        for _ in range(args.rounds):
            a.append(r.bytes_then_emitter(calls))
            b.append(r.text_from_device(r.lib.trt_render_host_ansi_half, r.half, calls))
            full.append(r.text_from_device(r.lib.trt_render_host_ansi, r.full, calls))
        cols = [spread([x[k] for x in a]) for k in range(4)]
        print(f"| {w}x{h} | {r.half.size} | {r.full.size} | {cols[0]} | {cols[1]} | {cols[2]} | {spread([x[0] for x in b])} | {spread([x[0] for x in full])} | "
              f"{'identical' if same else 'DIFFERENT'} |")
        passes.append(f"| {w}x{h} | {calls} | {cols[3]} | {spread([x[1] for x in full])} | {spread([x[1] for x in b])} |")
        ma, mb = statistics.median([x[0] for x in a]), statistics.median([x[0] for x in b])
        half_median, full_max = statistics.median([x[1] for x in b]), max(x[1] for x in full)
        verdicts.append(f"- {w}x{h}: route (b) takes {mb:.4f} ms per frame, route (a) {ma:.4f} ms: (b) is "
                        f"{'faster' if mb < ma else 'slower'} by {abs(ma - mb):.4f} ms ({abs(ma - mb) / ma * 100:.1f} % of (a)).  The half-block pass's "
                        f"reduce_ms median {half_median:.4f} lies {'not above' if half_median <= full_max else 'ABOVE'} the max of the full-text pass's rounds, {full_max:.4f}.")
        r.close()
    print("\nreduce_ms (trt_render_kernel_times: the pass behind the render kernel), median of a round's calls, then over the rounds:\n")
    print("| size | calls per round | bytes pass | full-text pass | half-block pass |")
    print("|---|---|---|---|---|")
    print("\n".join(passes))
    print("\n" + "\n".join(verdicts))


if __name__ == "__main__":
    main()
