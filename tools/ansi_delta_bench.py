"""What the terminal's text of a moving picture costs by two routes, for the demo scene on the reference's orbit (60 cameras, t = k / 60) at
480x280 and at 1920x1080, 10 bounces, 10 rays per pixel:

  (full)   trt_render_host_ansi: every cell of every frame, 25 bytes each, one copy across PCIe;
  (delta)  trt_render_host_ansi_delta: frame 0 as the same text, then only the records of the cells that changed (csrc/trt_ansi_delta.h): three
           small kernels behind the RGB8 form of the ordered mean, the length read back, then exactly that many bytes.

Within one process the two routes take turns, orbit by orbit, `--rounds` times (the spread of one route over the rounds stands beside the
difference between the two); per route and round the median, the least and the most over the orbit's frames 1..59 of bytes and of host-to-host
ms per frame (frame 0, the keyframe of the delta route, is listed by itself).  Then the three kernels by HIP events
(trt_ansi_delta_kernel_times): on the orbit's frames 0 -> 1, and on a 1920x1080 pair whose every cell changed with all neighbours different --
the longest text there is -- beside text_from_rgb8_kernel<ansi_text> (trt_ansi_from_rgb8_device) on the same frame.  Prints a markdown report
(profiles/r11/a_delta.md holds one)."""
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


def spread(values, digits=4):
    return f"{statistics.median(values):.{digits}f} (min {min(values):.{digits}f}, max {max(values):.{digits}f})"


class Orbit:
    def __init__(self, w, h):
        self.w, self.h = w, h
        self.lib = hip.lib()
        self.ctx = hip.Context(0)
        self.cams = [S.orbit_camera(k / 60.0, w, h) for k in range(FRAMES)]
        self.ctx.set_scene(S.demo_scene(S.synth_sky(256), self.cams[0]))
        self.structs = [hip.camera_struct(c) for c in self.cams]
        self.rows = hip.RowSet.whole(w, h)
        self.text = np.zeros(hip.ansi_delta_capacity(w, h), dtype=np.uint8)  # the caller's buffer, reused like main()'s
        self.full_bytes = hip.ansi_bytes(w, h)

    def full(self):
        """per frame: (bytes, host ms)"""
        out = []
        for cam in self.structs:
            t0 = time.perf_counter()
            hip._check(self.lib.trt_render_host_ansi(self.ctx._h, C.byref(cam), C.byref(self.rows), B, SPP, self.text.ctypes.data))
            out.append((self.full_bytes, (time.perf_counter() - t0) * 1e3))
        return out

    def delta(self):
        self.ctx.ansi_delta_reset()  # every orbit starts with its keyframe
        out, n = [], C.c_size_t(0)
        for cam in self.structs:
            t0 = time.perf_counter()
            hip._check(self.lib.trt_render_host_ansi_delta(self.ctx._h, C.byref(cam), C.byref(self.rows), B, SPP, self.text.ctypes.data, self.text.size, C.byref(n)))
            out.append((n.value, (time.perf_counter() - t0) * 1e3))
        return out

    def frames_rgb8(self, indices):
        return [self.ctx.render_host_rgb8(self.cams[k], self.rows, B, SPP) for k in indices]

    def close(self):
        self.ctx.close()


def kernel_times(ctx, shown, nxt, repeats=20):
    """(bytes of the delta text, [ms of measure, offsets, write] as medians over `repeats`, ms of text_from_rgb8_kernel<ansi_text> on `nxt`: wall clock over
    `repeats` launches back to back between two synchronisations)"""
    import torch
    rows, w, _ = shown.shape
    a, b = (torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).to("cuda:0") for f in (shown, nxt))
    room = torch.zeros(hip.ansi_delta_capacity(w, rows) + 8, dtype=torch.uint8, device="cuda:0")
    length = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    args = (a.data_ptr(), b.data_ptr(), w, rows, room.data_ptr(), room.numel() - 8, length.data_ptr())
    for _ in range(3):
        ctx.ansi_delta_kernel_times(*args)
    ms = [ctx.ansi_delta_kernel_times(*args) for _ in range(repeats)]
    for _ in range(3):
        ctx.ansi_from_rgb8(b.data_ptr(), w, rows, room.data_ptr())
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        ctx.ansi_from_rgb8(b.data_ptr(), w, rows, room.data_ptr())
    ctx.synchronize()
    whole = (time.perf_counter() - t0) / repeats * 1e3
    return int(length.cpu()[0]), [[m[k] for m in ms] for k in range(3)], whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--per-frame", action="store_true", help="also list every frame of the last round")
    args = ap.parse_args()
    print(f"# the terminal's text of the demo orbit, whole and as deltas: {FRAMES} cameras (t = k / 60), {B} bounces, {SPP} rays per pixel\n")
    print(f"(full) trt_render_host_ansi; (delta) trt_render_host_ansi_delta.  {args.rounds} rounds per size, an orbit of either route in turn within a round, "
          "after one orbit of each to warm up.  A cell: median over the frames 1..59 of the round (min, max).\n")
    kernels = []
    verdicts = []
    for w, h in SIZES:
        o = Orbit(w, h)
        o.full(), o.delta()
        rounds = [(o.full(), o.delta()) for _ in range(args.rounds)]
        print(f"## {w}x{h}: the whole text is {o.full_bytes} bytes\n")
        print("| round | (full) host ms per frame | (delta) bytes per frame | (delta) / (full) bytes | (delta) host ms per frame | (delta) frame 0, the keyframe: bytes, ms |")
        print("|---|---|---|---|---|---|")
        for i, (full, delta) in enumerate(rounds):
            ratio = [d[0] / o.full_bytes for d in delta[1:]]
            print(f"| {i} | {spread([f[1] for f in full[1:]])} | {spread([d[0] for d in delta[1:]], 0)} | {spread(ratio, 3)} | {spread([d[1] for d in delta[1:]])} | "
                  f"{delta[0][0]}, {delta[0][1]:.4f} |")
        mf = [statistics.median([f[1] for f in full[1:]]) for full, _ in rounds]
        md = [statistics.median([d[1] for d in delta[1:]]) for _, delta in rounds]
        verdicts.append(f"- {w}x{h}: medians per round, (full) {', '.join(f'{x:.4f}' for x in mf)} ms; (delta) {', '.join(f'{x:.4f}' for x in md)} ms: the delta route is "
                        f"{'faster' if max(md) < min(mf) else 'slower' if min(md) > max(mf) else 'within the spread of the rounds'} "
                        f"({statistics.median(md) - statistics.median(mf):+.4f} ms at the medians of the medians).")
        if args.per_frame:
            print("\n| frame | (full) ms | (delta) bytes | (delta) ms |\n|---|---|---|---|")
            for k, (f, d) in enumerate(zip(*rounds[-1])):
                print(f"| {k} | {f[1]:.4f} | {d[0]} | {d[1]:.4f} |")
        print()
        f0, f1 = o.frames_rgb8([0, 1])
        kernels.append((f"{w}x{h}, orbit frames 0 -> 1", kernel_times(o.ctx, f0, f1)))
        if (w, h) == SIZES[-1]:
            rng = np.random.default_rng(11)
            shown = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            nxt = shown ^ np.uint8(0x80)  # every cell changed; random colours: horizontal neighbours differ (but for one pair in 2^24)
            kernels.append((f"{w}x{h}, every cell changed, all neighbours different", kernel_times(o.ctx, shown, nxt)))
        o.close()
    print("## the three kernels (HIP events, median (min, max) of 20) beside text_from_rgb8_kernel<ansi_text> on the new frame (wall clock over 20 launches back to back)\n")
    print("| frames | delta text bytes | measure ms | offsets ms | write ms | sum ms | text_from_rgb8_kernel<ansi_text> ms (whole text) |")
    print("|---|---|---|---|---|---|---|")
    for what, (n, ms, whole) in kernels:
        total = [sum(x) for x in zip(*ms)]
        print(f"| {what} | {n} | {spread(ms[0])} | {spread(ms[1])} | {spread(ms[2])} | {spread(total)} | {whole:.4f} |")
    print("\n" + "\n".join(verdicts))


if __name__ == "__main__":
    main()
