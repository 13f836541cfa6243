"""What a host on a terminal with only the xterm 256-colour palette pays per frame for the two 256-colour texts (csrc/trt_ansi256.h: 13 bytes
a pixel; csrc/trt_ansi256_half.h: 11.5 bytes a pixel), beside their 24-bit counterparts, for the demo scene on its orbit (60 cameras, each
call the next) at 480x280 and at 1920x1080, 10 bounces, 10 rays per pixel, host-in/host-out, on one build in one run:

  (1) trt_render_host_ansi256 and trt_render_host_ansi256_half (the texts formed by the pass behind the render kernel);
  (2) trt_render_host_ansi and trt_render_host_ansi_half of the same build: the 24-bit texts, 25 and 19.5 bytes a pixel;
  (3) trt_render_host_rgb8 (3 bytes per pixel across PCIe) and trt_emitter_ansi256_half_rgb8 (the search and the formatting in a loop on the
      host): the route a host has without (1).

Route (3) makes a tenth of the other routes' calls per round.  The routes take turns round by round, so that the spread of one route over the rounds stands beside the difference between two.  Reported
with the spread: host ms per frame of every route (of (3) also its two halves), reduce_ms (trt_render_kernel_times) of the two new passes
beside that of the RGB8 pass, and whether (1)'s half-block text and (3)'s are identical.  Prints a markdown report
(profiles/r22/a_ansi256.md holds one)."""
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
SIZES = ((480, 280, 420), (1920, 1080, 60))  # width, height, calls per round: whole turns of the orbit
FRAMES = 60


def spread(values):
    return f"{statistics.median(values):.4f} (min {min(values):.4f}, max {max(values):.4f})"


class Routes:
    def __init__(self, w, h):
        self.w, self.h = w, h
        self.lib, self.hostlib = hip.lib(), host.lib()
        self.ctx = hip.Context(0)
        self.cams = [S.orbit_camera(k / 60.0, w, h) for k in range(FRAMES)]
        self.ctx.set_scene(S.demo_scene(S.synth_sky(256), self.cams[0]))
        self.structs = [hip.camera_struct(c) for c in self.cams]
        self.rows = hip.RowSet.whole(w, h)
        self.rgb = np.zeros((h, w, 3), dtype=np.uint8)  # the caller's buffers, reused like main()'s
        self.full256 = np.zeros(hip.ansi256_bytes(w, h), dtype=np.uint8)
        self.half256 = np.zeros(hip.ansi256_bytes(w, h, True), dtype=np.uint8)
        self.half256_on_host = np.zeros(hip.ansi256_bytes(w, h, True), dtype=np.uint8)
        self.half = np.zeros(hip.ansi_half_bytes(w, h), dtype=np.uint8)
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
        for k in range(calls):
            t0 = time.perf_counter()
            hip._check(self.lib.trt_render_host_rgb8(self.ctx._h, C.byref(self.structs[k % FRAMES]), C.byref(self.rows), B, SPP, self.rgb.ctypes.data))
            t1 = time.perf_counter()
            self.hostlib.trt_emitter_ansi256_half_rgb8(self.rgb.ctypes.data, self.w, self.h, self.half256_on_host.ctypes.data, self.half256_on_host.size, C.byref(n))
            emit += time.perf_counter() - t1
            render += t1 - t0
        return (render + emit) / calls * 1e3, render / calls * 1e3, emit / calls * 1e3, self.reduce_ms(calls)

    def text_from_device(self, entry, out, calls):
        """(host ms per frame, reduce_ms): the host entries end in a stream synchronise"""
        t0 = time.perf_counter()
        for k in range(calls):
            hip._check(entry(self.ctx._h, C.byref(self.structs[k % FRAMES]), C.byref(self.rows), B, SPP, out.ctypes.data))
        return (time.perf_counter() - t0) / calls * 1e3, self.reduce_ms(calls)

    def close(self):
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls-divisor", type=int, default=1, help="divide the calls per round (a shorter run)")
    args = ap.parse_args()
    print(f"# a frame as text in the xterm 256-colour palette beside the 24-bit texts, demo scene, {B} bounces, {SPP} rays per pixel\n")
    print("(1) trt_render_host_ansi256 and trt_render_host_ansi256_half; (2) trt_render_host_ansi and trt_render_host_ansi_half; "
          "(3) trt_render_host_rgb8 + trt_emitter_ansi256_half_rgb8.  "
          f"{args.rounds} rounds per size, the routes taking turns within a round; a cell is the median over the rounds (min, max), in ms.\n")
    print("| size | 256 full bytes | 256 half-block bytes | 24-bit full bytes | 24-bit half-block bytes | (1) full, host ms per frame | (1) half-block | "
          "(2) full | (2) half-block | (3) host ms per frame | (3) render call | (3) search and formatting on the host | (1)'s half-block text and (3)'s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    passes, verdicts = [], []
    for w, h, calls in SIZES:
        calls = max(calls // args.calls_divisor, 4)
        r = Routes(w, h)
        texts = ((r.lib.trt_render_host_ansi256, r.full256), (r.lib.trt_render_host_ansi256_half, r.half256), (r.lib.trt_render_host_ansi, r.full),
                 (r.lib.trt_render_host_ansi_half, r.half))
        for _ in range(10):  # every route's shapes warm before a timed round
            r.bytes_then_emitter(1)
            for entry, out in texts:
                r.text_from_device(entry, out, 1)
        same = r.half256_on_host.tobytes() == r.half256.tobytes()  # both of camera 0
        timed = [[] for _ in texts]
        three = []
        for _ in range(args.rounds):
            for k, (entry, out) in enumerate(texts):
                timed[k].append(r.text_from_device(entry, out, calls))
            three.append(r.bytes_then_emitter(max(calls // 10, 4)))  # a tenth of the calls: the host's search takes a quarter of a microsecond a pixel
        cols = [spread([x[k] for x in three]) for k in range(4)]
        print(f"| {w}x{h} | {r.full256.size} | {r.half256.size} | {r.full.size} | {r.half.size} | " + " | ".join(spread([x[0] for x in t]) for t in timed) +
              f" | {cols[0]} | {cols[1]} | {cols[2]} | {'identical' if same else 'DIFFERENT'} |")
        passes.append(f"| {w}x{h} | {calls} | {cols[3]} | " + " | ".join(spread([x[1] for x in t]) for t in timed) + " |")
        m = [statistics.median([x[0] for x in t]) for t in timed]
        m3 = statistics.median([x[0] for x in three])
        verdicts.append(f"- {w}x{h}: the 256-colour full text takes {m[0]:.4f} ms per frame, the 24-bit full text {m[2]:.4f} "
                        f"({'FASTER' if m[0] < m[2] else 'NOT faster'}: {m[2] / m[0]:.2f} x the time for {r.full.size / r.full256.size:.2f} x the bytes); "
                        f"the 256-colour half-block text {m[1]:.4f}, the 24-bit half-block text {m[3]:.4f} "
                        f"({'FASTER' if m[1] < m[3] else 'NOT faster'}: {m[3] / m[1]:.2f} x the time for {r.half.size / r.half256.size:.2f} x the bytes); "
                        f"RGB8 bytes and the host's search and formatter {m3:.4f} ({m3 / m[1]:.2f} x the device's half-block route).")
        r.close()
    print("\nreduce_ms (trt_render_kernel_times: the pass behind the render kernel), median of a round's calls, then over the rounds:\n")
    print("| size | calls per round | RGB8 pass | 256 full pass | 256 half-block pass | 24-bit full pass | 24-bit half-block pass |")
    print("|---|---|---|---|---|---|---|")
    print("\n".join(passes))
    print("\n" + "\n".join(verdicts))


if __name__ == "__main__":
    main()
