"""What a host whose only consumer is a SIXEL terminal pays per frame for a DEC sixel image (csrc/trt_sixel.h: the 240 fixed colours of the
xterm palette, bands of six rows, a colour row per colour of a band), beside the other routes to a terminal, for the demo scene on its orbit
(60 cameras, each call the next) at 480x280 and at 1920x1080, 10 bounces, 10 rays per pixel, host-in/host-out, on one build in one run:

  (1) trt_render_host_sixel (the image formed by three kernels behind the RGB8 form of the ordered mean, nothing left to do);
  (2) trt_render_host_rgb8 (3 bytes per pixel across PCIe) and trt_emitter_sixel_rgb8 (a search of 240 palette entries per pixel on the
      host): the route a host has without (1) -- few calls per round, the search takes seconds per 1080p frame;
  (3) trt_render_host_kitty (4.01 bytes a pixel) and trt_render_host_ansi_half (19.5 bytes a pixel), for scale.

The routes take turns round by round, so that the spread of one route over the rounds stands beside the difference between two.  Reported
with the spread: host ms per frame of every route (of (2) also its two halves), the image's bytes a pixel and colours a band over the orbit,
whether (1)'s text and (2)'s are identical, reduce_ms (trt_render_kernel_times) of the RGB8 pass, and the device time of the image's three
kernels together (HIP events around trt_sixel_from_rgb8_device of a frame in device memory).  Prints a markdown report
(profiles/r23/a_sixel.md holds one)."""
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
SIZES = ((480, 280, 420, 12), (1920, 1080, 60, 2))  # width, height, calls per round of the device routes (whole turns of the orbit), of route (2)
FRAMES = 60


def spread(values, digits=4):
    return f"{statistics.median(values):.{digits}f} (min {min(values):.{digits}f}, max {max(values):.{digits}f})"


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
        self.sixel = np.zeros(hip.sixel_capacity(w, h), dtype=np.uint8)
        self.sixel_on_host = np.zeros(hip.sixel_capacity(w, h), dtype=np.uint8)
        self.kitty = np.zeros(hip.kitty_bytes(w, h), dtype=np.uint8)
        self.half = np.zeros(hip.ansi_half_bytes(w, h), dtype=np.uint8)
        self.lengths = []  # of the images of route (1), every call

    def reduce_ms(self, calls):
        n = min(calls, 256)
        a, b = (C.c_float * n)(), (C.c_float * n)()
        got = self.lib.trt_render_kernel_times(self.ctx._h, a, b, n)
        return statistics.median(b[:got])

    def image_from_device(self, calls):
        """(host ms per frame, reduce_ms of the bytes pass in front of the image's kernels)"""
        n = C.c_size_t(0)
        t0 = time.perf_counter()
        for k in range(calls):
            hip._check(self.lib.trt_render_host_sixel(self.ctx._h, C.byref(self.structs[k % FRAMES]), C.byref(self.rows), B, SPP, self.sixel.ctypes.data, self.sixel.size,
                                                      C.byref(n)))
            self.lengths.append(n.value)
        return (time.perf_counter() - t0) / calls * 1e3, self.reduce_ms(calls)

    def bytes_then_emitter(self, calls):
        """(host ms per frame, of which the render call, of which the emitter, reduce_ms of the bytes pass, the last text's length)"""
        render = emit = 0.0
        n = C.c_size_t(0)
        for k in range(calls):
            t0 = time.perf_counter()
            hip._check(self.lib.trt_render_host_rgb8(self.ctx._h, C.byref(self.structs[k % FRAMES]), C.byref(self.rows), B, SPP, self.rgb.ctypes.data))
            t1 = time.perf_counter()
            self.hostlib.trt_emitter_sixel_rgb8(self.rgb.ctypes.data, self.w, self.h, self.sixel_on_host.ctypes.data, self.sixel_on_host.size, C.byref(n))
            emit += time.perf_counter() - t1
            render += t1 - t0
        return (render + emit) / calls * 1e3, render / calls * 1e3, emit / calls * 1e3, self.reduce_ms(calls), n.value

    def text_from_device(self, entry, out, calls):
        t0 = time.perf_counter()
        for k in range(calls):
            hip._check(entry(self.ctx._h, C.byref(self.structs[k % FRAMES]), C.byref(self.rows), B, SPP, out.ctypes.data))
        return (time.perf_counter() - t0) / calls * 1e3

    def kernels_ms(self, repeats=20):
        """device ms of measure + offsets + write together, by events on the context's stream, of camera 0's frame in device memory"""
        import torch
        frame = torch.zeros(self.w * self.h * 3, dtype=torch.uint8, device="cuda:0")
        text = torch.zeros(self.sixel.size, dtype=torch.uint8, device="cuda:0")
        length = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        stream = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        self.ctx.set_stream(stream.cuda_stream)
        self.ctx.render_device_rgb8(self.cams[0], self.rows, B, SPP, frame.data_ptr(), frame.numel())
        times = []
        for _ in range(repeats + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            self.ctx.sixel_from_rgb8(frame.data_ptr(), self.w, self.h, text.data_ptr(), text.numel(), length.data_ptr())
            b.record(stream)
            stream.synchronize()
            times.append(a.elapsed_time(b))
        self.ctx.set_stream(0)
        return times[3:]

    def close(self):
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls-divisor", type=int, default=1, help="divide the calls per round (a shorter run)")
    args = ap.parse_args()
    print(f"# a frame as a DEC sixel image beside the other routes to a terminal, demo scene, {B} bounces, {SPP} rays per pixel\n")
    print("(1) trt_render_host_sixel; (2) trt_render_host_rgb8 + trt_emitter_sixel_rgb8; (3) trt_render_host_kitty and trt_render_host_ansi_half.  "
          f"{args.rounds} rounds per size, the routes taking turns within a round; a cell is the median over the rounds (min, max), in ms.\n")
    print("| size | (1) host ms per frame | (2) host ms per frame | (2) render call | (2) palette search and formatting on the host | "
          "(3) kitty image, host ms per frame | (3) half-block text, host ms per frame | (1)'s text and (2)'s |")
    print("|---|---|---|---|---|---|---|---|")
    sizes, passes, verdicts = [], [], []
    for w, h, calls, host_calls in SIZES:
        calls, host_calls = max(calls // args.calls_divisor, 4), max(host_calls // args.calls_divisor, 1)
        r = Routes(w, h)
        texts = ((r.lib.trt_render_host_kitty, r.kitty), (r.lib.trt_render_host_ansi_half, r.half))
        for _ in range(10):  # every device route's shapes warm before a timed round
            r.image_from_device(1)
            for entry, out in texts:
                r.text_from_device(entry, out, 1)
        length_of_two = r.bytes_then_emitter(1)[4]  # both of camera 0
        same = r.lengths[-1] == length_of_two and r.sixel_on_host[:length_of_two].tobytes() == r.sixel[:length_of_two].tobytes()
        r.lengths.clear()
        one, two, kitty, half = [], [], [], []
        for _ in range(args.rounds):
            one.append(r.image_from_device(calls))
            two.append(r.bytes_then_emitter(host_calls))
            kitty.append(r.text_from_device(*texts[0], calls))
            half.append(r.text_from_device(*texts[1], calls))
        kernels = r.kernels_ms()
        cols = [spread([x[k] for x in two], 3) for k in range(3)]
        print(f"| {w}x{h} | {spread([x[0] for x in one])} | {cols[0]} | {cols[1]} | {cols[2]} | {spread(kitty)} | {spread(half)} | {'identical' if same else 'DIFFERENT'} |")
        row_len, bands = 4 + w + 1 + (-(w + 1)) % 4, (h + 5) // 6
        per_pixel = [n / (w * h) for n in r.lengths]
        per_band = [(n - 4352) / row_len / bands for n in r.lengths]
        sizes.append(f"| {w}x{h} | {calls} | {host_calls} | {hip.sixel_capacity(w, h)} | {int(statistics.median(r.lengths))} (min {min(r.lengths)}, max {max(r.lengths)}) | "
                     f"{spread(per_pixel, 3)} | {spread(per_band, 1)} | {r.kitty.size} | {r.half.size} |")
        passes.append(f"| {w}x{h} | {spread([x[1] for x in one])} | {spread([x[3] for x in two])} | {spread(kernels)} |")
        m1, m2 = statistics.median([x[0] for x in one]), statistics.median([x[0] for x in two])
        verdicts.append(f"- {w}x{h}: route (1) takes {m1:.4f} ms per frame, route (2) {m2:.3f} ms: the device route is {'faster' if m1 < m2 else 'SLOWER'} by a factor of "
                        f"{max(m1, m2) / min(m1, m2):.1f}; the kitty image {statistics.median(kitty):.4f} ms, the half-block text {statistics.median(half):.4f} ms.")
        r.close()
    print("\nThe image over the orbit (every call of route (1) in the timed rounds): its length depends on the picture.\n")
    print("| size | calls per round, device routes | calls per round, route (2) | capacity | image bytes | bytes a pixel | colours a band | kitty image bytes | half-block bytes |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("\n".join(sizes))
    print("\nDevice time: reduce_ms (trt_render_kernel_times: the RGB8 form of the ordered mean, behind the render kernel) of the calls of routes (1) and (2), "
          "median of a round's calls, then over the rounds; and measure + offsets + write together by HIP events, of one frame in device memory, 20 times:\n")
    print("| size | RGB8 pass in route (1) | RGB8 pass in route (2) | the image's three kernels |")
    print("|---|---|---|---|")
    print("\n".join(passes))
    print("\n" + "\n".join(verdicts))


if __name__ == "__main__":
    main()
