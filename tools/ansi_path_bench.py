"""What a host whose only consumer is the terminal pays per frame for the text it writes, by two routes, for the demo scene at 480x280 and at
1920x1080, 10 bounces, 10 rays per pixel:

  (a) trt_render_host_rgb8 (3 bytes per pixel across PCIe) and trt_emitter_patch_rgb8 (the digits formatted in a loop on the host);
  (b) trt_render_host_ansi (the text formatted by the pass behind the render kernel, 25 bytes per pixel across PCIe, nothing left to do).

The two take turns round by round, so that the spread of one route over the rounds stands beside the difference between the two.  Reported
with the spread: host ms per frame of either route (of (a) also its two halves), reduce_ms (trt_render_kernel_times) of the bytes pass and of
the text pass, and whether (a)'s emitter buffer and (b)'s text are identical.  Prints a markdown report (profiles/r10/a_ansi.md holds one)."""
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
        self.rgb = np.zeros((h, w, 3), dtype=np.uint8)
        self.text = np.zeros(hip.ansi_bytes(w, h), dtype=np.uint8)  # the caller's buffers, reused like main()'s
        self.emitter = host.Emitter(w, h)

    def reduce_ms(self, calls):
        n = min(calls, 256)
        a, b = (C.c_float * n)(), (C.c_float * n)()
        got = self.lib.trt_render_kernel_times(self.ctx._h, a, b, n)
        return statistics.median(b[:got])

    def bytes_then_emitter(self, calls):
        """(host ms per frame, of which the render call, of which the emitter, reduce_ms)"""
        render = patch = 0.0
        for _ in range(calls):
            t0 = time.perf_counter()
            hip._check(self.lib.trt_render_host_rgb8(self.ctx._h, C.byref(self.cam), C.byref(self.rows), B, SPP, self.rgb.ctypes.data))
            t1 = time.perf_counter()
            self.hostlib.trt_emitter_patch_rgb8(self.emitter._h, self.rgb.ctypes.data)
            patch += time.perf_counter() - t1
            render += t1 - t0
        return (render + patch) / calls * 1e3, render / calls * 1e3, patch / calls * 1e3, self.reduce_ms(calls)

    def text_from_device(self, calls):
        """(host ms per frame, reduce_ms)"""
        t0 = time.perf_counter()
        for _ in range(calls):
            hip._check(self.lib.trt_render_host_ansi(self.ctx._h, C.byref(self.cam), C.byref(self.rows), B, SPP, self.text.ctypes.data))
        return (time.perf_counter() - t0) / calls * 1e3, self.reduce_ms(calls)

    def close(self):
        self.emitter.close()
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    print(f"# the terminal's text of a frame by two routes, demo scene, {B} bounces, {SPP} rays per pixel\n")
    print("(a) trt_render_host_rgb8 + trt_emitter_patch_rgb8; (b) trt_render_host_ansi.  "
          f"{args.rounds} rounds per size, the routes taking turns within a round; a cell is the median over the rounds (min, max), in ms.\n")
    print("| size | text bytes | (a) host ms per frame | (a) render call | (a) emitter on the host | (b) host ms per frame | reduce_ms, bytes pass | reduce_ms, text pass | (a)'s buffer and (b)'s text |")
    print("|---|---|---|---|---|---|---|---|---|")
    verdicts = []
    for w, h, calls in SIZES:
        r = Routes(w, h)
        for _ in range(10):
            r.bytes_then_emitter(1)
            r.text_from_device(1)
        same = r.emitter.bytes() == r.text.tobytes()
        a, b = [], []
        for _ in range(args.rounds):
            a.append(r.bytes_then_emitter(calls))
            b.append(r.text_from_device(calls))
        cols = [spread([x[k] for x in a]) for k in range(4)]
        print(f"| {w}x{h} | {r.text.size} | {cols[0]} | {cols[1]} | {cols[2]} | {spread([x[0] for x in b])} | {cols[3]} | {spread([x[1] for x in b])} | "
              f"{'identical' if same else 'DIFFERENT'} |")
        ma, mb = statistics.median([x[0] for x in a]), statistics.median([x[0] for x in b])
        verdicts.append(f"- {w}x{h}: route (b) takes {mb:.4f} ms per frame, route (a) {ma:.4f} ms: (b) is "
                        f"{'faster' if mb < ma else 'slower'} by {abs(ma - mb):.4f} ms ({abs(ma - mb) / ma * 100:.1f} % of (a)).")
        r.close()
    print("\n" + "\n".join(verdicts))


if __name__ == "__main__":
    main()
