"""What a host whose only consumer is the terminal pays per frame for a KITTY GRAPHICS-PROTOCOL image (csrc/trt_kitty.h: base64 of the RGB
bytes, 4.01 bytes of text a pixel), beside the other routes to a terminal, for the demo scene on its orbit (60 cameras, each call the next)
at 480x280 and at 1920x1080, 10 bounces, 10 rays per pixel, host-in/host-out, on one build in one run:

  (1) trt_render_host_kitty (the image text formed by the pass behind the render kernel, nothing left to do);
  (2) trt_render_host_rgb8 (3 bytes per pixel across PCIe) and trt_emitter_kitty_rgb8 (base64 in a loop on the host): the route a host has
      without (1);
  (3) trt_render_host_ansi_half (19.5 bytes a pixel) and trt_render_host_ansi (25 bytes a pixel): the character-cell texts.

The routes take turns round by round, so that the spread of one route over the rounds stands beside the difference between two.  Reported
with the spread: host ms per frame of every route (of (2) also its two halves), reduce_ms (trt_render_kernel_times) of the kitty pass
beside that of the RGB8 pass, and whether (1)'s text and (2)'s are identical.  Prints a markdown report (profiles/r21/a_kitty.md holds
one)."""
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
        self.kitty = np.zeros(hip.kitty_bytes(w, h), dtype=np.uint8)
        self.kitty_on_host = np.zeros(hip.kitty_bytes(w, h), dtype=np.uint8)
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
            self.hostlib.trt_emitter_kitty_rgb8(self.rgb.ctypes.data, self.w, self.h, self.kitty_on_host.ctypes.data, self.kitty_on_host.size, C.byref(n))
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
    print(f"# a frame as a kitty graphics-protocol image beside the other routes to a terminal, demo scene, {B} bounces, {SPP} rays per pixel\n")
    print("(1) trt_render_host_kitty; (2) trt_render_host_rgb8 + trt_emitter_kitty_rgb8; (3) trt_render_host_ansi_half and trt_render_host_ansi.  "
          f"{args.rounds} rounds per size, the routes taking turns within a round; a cell is the median over the rounds (min, max), in ms.\n")
    print("| size | image bytes | half-block bytes | full text bytes | (1) host ms per frame | (2) host ms per frame | (2) render call | (2) base64 on the host | "
          "(3) half-block, host ms per frame | (3) full text, host ms per frame | (1)'s text and (2)'s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    passes, verdicts = [], []
    for w, h, calls in SIZES:
        calls = max(calls // args.calls_divisor, 4)
        r = Routes(w, h)
        texts = ((r.lib.trt_render_host_kitty, r.kitty), (r.lib.trt_render_host_ansi_half, r.half), (r.lib.trt_render_host_ansi, r.full))
        for _ in range(10):  # every route's shapes warm before a timed round
            r.bytes_then_emitter(1)
            for entry, out in texts:
                r.text_from_device(entry, out, 1)
        same = r.kitty_on_host.tobytes() == r.kitty.tobytes()  # both of camera 0
        one, two, half, full = [], [], [], []
        for _ in range(args.rounds):
            one.append(r.text_from_device(*texts[0], calls))
            two.append(r.bytes_then_emitter(calls))
            half.append(r.text_from_device(*texts[1], calls))
            full.append(r.text_from_device(*texts[2], calls))
        cols = [spread([x[k] for x in two]) for k in range(4)]
        print(f"| {w}x{h} | {r.kitty.size} | {r.half.size} | {r.full.size} | {spread([x[0] for x in one])} | {cols[0]} | {cols[1]} | {cols[2]} | "
              f"{spread([x[0] for x in half])} | {spread([x[0] for x in full])} | {'identical' if same else 'DIFFERENT'} |")
        passes.append(f"| {w}x{h} | {calls} | {cols[3]} | {spread([x[1] for x in one])} | {spread([x[1] for x in half])} | {spread([x[1] for x in full])} |")
        m1, m2, mh, mf = (statistics.median([x[0] for x in xs]) for xs in (one, two, half, full))
        kitty_pass, bytes_rounds = statistics.median([x[1] for x in one]), [x[3] for x in two]
        inside = min(bytes_rounds) <= kitty_pass <= max(bytes_rounds)
        verdicts.append(f"- {w}x{h}: route (1) takes {m1:.4f} ms per frame; route (2) {m2:.4f} ms ((1) is {'faster' if m1 < m2 else 'slower'} by {abs(m2 - m1):.4f} ms); "
                        f"the half-block text {mh:.4f} ms ({mh / m1:.2f} x (1), {r.half.size / r.kitty.size:.2f} x the bytes), the full text {mf:.4f} ms "
                        f"({mf / m1:.2f} x (1), {r.full.size / r.kitty.size:.2f} x the bytes).  The kitty pass's reduce_ms median {kitty_pass:.4f} lies "
                        f"{'within' if inside else 'below' if kitty_pass < min(bytes_rounds) else 'ABOVE'} the RGB8 pass's rounds, {min(bytes_rounds):.4f} .. {max(bytes_rounds):.4f}.")
        r.close()
    print("\nreduce_ms (trt_render_kernel_times: the pass behind the render kernel), median of a round's calls, then over the rounds:\n")
    print("| size | calls per round | RGB8 pass | kitty pass | half-block pass | full-text pass |")
    print("|---|---|---|---|---|---|")
    print("\n".join(passes))
    print("\n" + "\n".join(verdicts))


if __name__ == "__main__":
    main()
