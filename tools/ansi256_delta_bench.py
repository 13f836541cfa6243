"""What the terminal's text of a moving picture costs in the xterm 256-colour palette, whole and as deltas, beside the 24-bit delta texts, for
the demo scene on the reference's orbit (60 cameras, t = k / 60) at 480x280 and at 1920x1080, 10 bounces, 10 rays per pixel, in full cells and
in half-block cells:

  (whole256)  trt_render_host_ansi256[_half]: every cell of every frame, 13 (half-block: 23) bytes each, one copy across PCIe;
  (delta256)  trt_render_host_ansi256_delta[_half]: frame 0 as that text, then the records of the cells whose palette ENTRY changed
              (csrc/trt_ansi256_delta.h, trt_ansi256_delta_half.h): three small kernels behind the RGB8 form of the ordered mean, the
              length read back, then exactly that many bytes;
  (delta24)   trt_render_host_ansi_delta[_half]: the same route in 24-bit colour, whose records are of the cells whose BYTES changed.

Within one process the three routes take turns, orbit by orbit, `--rounds` times after one orbit of each to warm up (the spread of one route
over the rounds stands beside the differences between the routes); per route and round the median, the least and the most over the orbit's
frames 1..59 of bytes and of host-to-host ms per frame.  Then the three kernels by HIP events (trt_ansi256_delta[_half]_kernel_times beside
trt_ansi_delta[_half]_kernel_times) on the orbit's frames 0 -> 1, 20 repeats after 3.  Prints a markdown report (profiles/r26/a_delta256.md
holds one)."""
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

B, SPP, FRAMES = 10, 10, 60
SIZES = ((480, 280), (1920, 1080))
ROUTES = ("whole256", "delta256", "delta24")


def spread(values, digits=4):
    return f"{statistics.median(values):.{digits}f} (min {min(values):.{digits}f}, max {max(values):.{digits}f})"


class Orbit:
    def __init__(self, w, h, half):
        self.w, self.h, self.half = w, h, half
        self.lib = hip.lib()
        self.ctx = hip.Context(0)
        self.cams = [S.orbit_camera(k / 60.0, w, h) for k in range(FRAMES)]
        self.ctx.set_scene(S.demo_scene(S.synth_sky(256), self.cams[0]))
        self.structs = [hip.camera_struct(c) for c in self.cams]
        self.rows = hip.RowSet.whole(w, h)
        suffix = "_half" if half else ""
        self.whole_bytes = hip.ansi256_bytes(w, h, half=half)
        room = max(hip.ansi256_delta_capacity(w, h, half=half), hip.ansi_delta_half_capacity(w, h) if half else hip.ansi_delta_capacity(w, h))
        self.text = np.zeros(room, dtype=np.uint8)  # the caller's buffer, reused like main()'s
        self.entries = {"whole256": getattr(self.lib, "trt_render_host_ansi256" + suffix), "delta256": getattr(self.lib, "trt_render_host_ansi256_delta" + suffix),
                        "delta24": getattr(self.lib, "trt_render_host_ansi_delta" + suffix)}

    def orbit(self, route):
        """per frame: (bytes, host ms)"""
        out, n = [], C.c_size_t(0)
        self.ctx.ansi_delta_reset()  # every orbit of a delta route starts with its keyframe
        for cam in self.structs:
            t0 = time.perf_counter()
            if route == "whole256":
                hip._check(self.entries[route](self.ctx._h, C.byref(cam), C.byref(self.rows), B, SPP, self.text.ctypes.data))
                n.value = self.whole_bytes
            else:
                hip._check(self.entries[route](self.ctx._h, C.byref(cam), C.byref(self.rows), B, SPP, self.text.ctypes.data, self.text.size, C.byref(n)))
            out.append((n.value, (time.perf_counter() - t0) * 1e3))
        return out

    def frames_rgb8(self, indices):
        return [self.ctx.render_host_rgb8(self.cams[k], self.rows, B, SPP) for k in indices]

    def close(self):
        self.ctx.close()


def kernel_times(ctx, shown, nxt, half, palette, repeats=20):
    """(bytes of the delta text, [ms of measure, offsets, write] over `repeats` calls after 3) of the palette's or the 24-bit kind's kernels"""
    import torch
    rows, w, _ = shown.shape
    a, b = (torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).to("cuda:0") for f in (shown, nxt))
    capacity = hip.ansi256_delta_capacity(w, rows, half=half) if palette else (hip.ansi_delta_half_capacity if half else hip.ansi_delta_capacity)(w, rows)
    room = torch.zeros(capacity + 8, dtype=torch.uint8, device="cuda:0")
    length = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    args = (a.data_ptr(), b.data_ptr(), w, rows, room.data_ptr(), capacity, length.data_ptr())
    if palette:
        timed = lambda: ctx.ansi256_delta_kernel_times(*args, half=half)
    else:
        timed = lambda: (ctx.ansi_delta_half_kernel_times if half else ctx.ansi_delta_kernel_times)(*args)
    for _ in range(3):
        timed()
    ms = [timed() for _ in range(repeats)]
    return int(length.cpu()[0]), [[m[k] for m in ms] for k in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print(f"# the terminal's text of the demo orbit in the xterm 256-colour palette, whole and as deltas: {FRAMES} cameras (t = k / 60), {B} bounces, {SPP} rays per pixel\n")
    print("(whole256) trt_render_host_ansi256[_half]; (delta256) trt_render_host_ansi256_delta[_half]; (delta24) trt_render_host_ansi_delta[_half].  "
          f"{args.rounds} rounds per size and shape of cell, an orbit of each route in turn within a round, after one orbit of each to warm up.  "
          "A cell: median over the frames 1..59 of the round (min, max); host-in/host-out ms per frame.\n")
    kernels, verdicts = [], []
    for w, h in SIZES:
        for half in (False, True):
            cells = "half-block cells" if half else "full cells"
            o = Orbit(w, h, half)
            for route in ROUTES:
                o.orbit(route)
            rounds = [{route: o.orbit(route) for route in ROUTES} for _ in range(args.rounds)]
            print(f"## {w}x{h}, {cells}: the whole 256-colour text is {o.whole_bytes} bytes\n")
            print("| round | (whole256) ms | (delta256) bytes | (delta256) / (whole256) bytes | (delta256) ms | (delta24) bytes | (delta256) / (delta24) bytes | (delta24) ms | "
                  "(delta256) frame 0, the keyframe: bytes, ms |")
            print("|---|---|---|---|---|---|---|---|---|")
            for i, r in enumerate(rounds):
                d256, d24 = r["delta256"][1:], r["delta24"][1:]
                print(f"| {i} | {spread([f[1] for f in r['whole256'][1:]])} | {spread([d[0] for d in d256], 0)} | {spread([d[0] / o.whole_bytes for d in d256], 3)} | "
                      f"{spread([d[1] for d in d256])} | {spread([d[0] for d in d24], 0)} | {spread([a[0] / max(b[0], 1) for a, b in zip(d256, d24)], 3)} | "
                      f"{spread([d[1] for d in d24])} | {r['delta256'][0][0]}, {r['delta256'][0][1]:.4f} |")
            med = {route: [statistics.median([f[1] for f in r[route][1:]]) for r in rounds] for route in ROUTES}
            size = {route: statistics.median([f[0] for r in rounds for f in r[route][1:]]) for route in ROUTES}

            def against(other):
                mine, theirs = med["delta256"], med[other]
                word = "faster than" if max(mine) < min(theirs) else "slower than" if min(mine) > max(theirs) else "within the spread of the rounds of"
                return f"{word} ({other}) ({statistics.median(mine) - statistics.median(theirs):+.4f} ms at the medians of the medians)"

            verdicts.append(f"- {w}x{h}, {cells}: bytes per frame at the median (whole256) {size['whole256']:.0f}, (delta256) {size['delta256']:.0f}, (delta24) {size['delta24']:.0f}; "
                            f"ms per frame, medians per round, " + "; ".join(f"({route}) {', '.join(f'{x:.4f}' for x in med[route])}" for route in ROUTES) +
                            f": (delta256) is {against('whole256')} and {against('delta24')}.")
            print()
            f0, f1 = o.frames_rgb8([0, 1])
            kernels.append((f"{w}x{h}, {cells}, (delta256)", kernel_times(o.ctx, f0, f1, half, True)))
            kernels.append((f"{w}x{h}, {cells}, (delta24)", kernel_times(o.ctx, f0, f1, half, False)))
            o.close()
    print("## the three kernels on the orbit's frames 0 -> 1 (HIP events, median (min, max) of 20 after 3)\n")
    print("| frames | delta text bytes | measure ms | offsets ms | write ms | sum ms |")
    print("|---|---|---|---|---|---|")
    for what, (n, ms) in kernels:
        total = [sum(x) for x in zip(*ms)]
        print(f"| {what} | {n} | {spread(ms[0])} | {spread(ms[1])} | {spread(ms[2])} | {spread(total)} |")
    print("\n" + "\n".join(verdicts))


if __name__ == "__main__":
    main()
