"""What the terminal's half-block text of a moving picture costs whole and as deltas, for the demo scene on the reference's orbit (60 cameras,
t = k / 60) at 480x280 and at 1920x1080, 10 bounces, 10 rays per pixel:

  (half)        trt_render_host_ansi_half: every cell of every frame, 39 bytes for two pixels, one copy across PCIe;
  (delta)       trt_render_host_ansi_delta: the full text's delta, two-column cells of one pixel (csrc/trt_ansi_delta.h);
  (delta half)  trt_render_host_ansi_delta_half: frame 0 as the half-block text, then only the records of the cells either of whose two
                pixels changed (csrc/trt_ansi_delta_half.h): three small kernels behind the RGB8 form of the ordered mean, the length read
                back, then exactly that many bytes.

Within one process the three routes take turns, orbit by orbit, `--rounds` times (the spread of one route over the rounds stands beside the
differences between them); per route and round the median, the least and the most over the orbit's frames 1..59 of bytes and of host-to-host
ms per frame (frame 0, the keyframe of the delta routes, is listed by itself).  Then the three kernels by HIP events
(trt_ansi_delta_half_kernel_times): on the orbit's frames 0 -> 1, and on a 1920x1080 pair whose every cell changed with all neighbours
different -- the longest text there is -- beside text_from_rgb8_kernel<ansi_half_text> (trt_ansi_half_from_rgb8_device) on the same frame.  Prints a
markdown report (profiles/r15/a_delta_half.md holds one)."""
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
        self.text = np.zeros(max(hip.ansi_delta_capacity(w, h), hip.ansi_delta_half_capacity(w, h)), dtype=np.uint8)  # the caller's buffer, reused like main()'s
        self.half_bytes = hip.ansi_half_bytes(w, h)

    def half(self):
        """per frame: (bytes, host ms)"""
        out = []
        for cam in self.structs:
            t0 = time.perf_counter()
            hip._check(self.lib.trt_render_host_ansi_half(self.ctx._h, C.byref(cam), C.byref(self.rows), B, SPP, self.text.ctypes.data))
            out.append((self.half_bytes, (time.perf_counter() - t0) * 1e3))
        return out

    def _delta(self, entry):
        self.ctx.ansi_delta_reset()  # every orbit starts with its keyframe
        out, n = [], C.c_size_t(0)
        for cam in self.structs:
            t0 = time.perf_counter()
            hip._check(entry(self.ctx._h, C.byref(cam), C.byref(self.rows), B, SPP, self.text.ctypes.data, self.text.size, C.byref(n)))
            out.append((n.value, (time.perf_counter() - t0) * 1e3))
        return out

    def delta(self):
        return self._delta(self.lib.trt_render_host_ansi_delta)

    def delta_half(self):
        return self._delta(self.lib.trt_render_host_ansi_delta_half)

    def frames_rgb8(self, indices):
        return [self.ctx.render_host_rgb8(self.cams[k], self.rows, B, SPP) for k in indices]

    def close(self):
        self.ctx.close()


def kernel_times(ctx, shown, nxt, repeats=20):
    """(bytes of the delta text, [ms of measure, offsets, write] as medians over `repeats`, ms of text_from_rgb8_kernel<ansi_half_text> on `nxt`: wall
    clock over `repeats` launches back to back between two synchronisations)"""
    import torch
    rows, w, _ = shown.shape
    a, b = (torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).to("cuda:0") for f in (shown, nxt))
    room = torch.zeros(hip.ansi_delta_half_capacity(w, rows) + 8, dtype=torch.uint8, device="cuda:0")
    length = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    args = (a.data_ptr(), b.data_ptr(), w, rows, room.data_ptr(), room.numel() - 8, length.data_ptr())
    for _ in range(3):
        ctx.ansi_delta_half_kernel_times(*args)
    ms = [ctx.ansi_delta_half_kernel_times(*args) for _ in range(repeats)]
    for _ in range(3):
        ctx.ansi_half_from_rgb8(b.data_ptr(), w, rows, room.data_ptr())
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        ctx.ansi_half_from_rgb8(b.data_ptr(), w, rows, room.data_ptr())
    ctx.synchronize()
    whole = (time.perf_counter() - t0) / repeats * 1e3
    return int(length.cpu()[0]), [[m[k] for m in ms] for k in range(3)], whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print(f"# the terminal's half-block text of the demo orbit, whole and as deltas: {FRAMES} cameras (t = k / 60), {B} bounces, {SPP} rays per pixel\n")
    print(f"(half) trt_render_host_ansi_half; (delta) trt_render_host_ansi_delta; (delta half) trt_render_host_ansi_delta_half.  {args.rounds} rounds per size, an "
          "orbit of each route in turn within a round, after one orbit of each to warm up.  A cell: median over the frames 1..59 of the round (min, max).\n")
    kernels = []
    verdicts = []
    for w, h in SIZES:
        o = Orbit(w, h)
        o.half(), o.delta(), o.delta_half()
        rounds = [(o.half(), o.delta(), o.delta_half()) for _ in range(args.rounds)]
        print(f"## {w}x{h}: the whole half-block text is {o.half_bytes} bytes, the whole full text {hip.ansi_bytes(w, h)}\n")
        print("| round | (half) host ms per frame | (delta) bytes per frame | (delta) host ms per frame | (delta half) bytes per frame | (delta half) / (half) bytes | "
              "(delta half) host ms per frame | (delta half) frame 0, the keyframe: bytes, ms |")
        print("|---|---|---|---|---|---|---|---|")
        for i, (half, delta, dh) in enumerate(rounds):
            ratio = [d[0] / o.half_bytes for d in dh[1:]]
            print(f"| {i} | {spread([f[1] for f in half[1:]])} | {spread([d[0] for d in delta[1:]], 0)} | {spread([d[1] for d in delta[1:]])} | "
                  f"{spread([d[0] for d in dh[1:]], 0)} | {spread(ratio, 3)} | {spread([d[1] for d in dh[1:]])} | {dh[0][0]}, {dh[0][1]:.4f} |")
        mh, md, mdh = ([statistics.median([f[1] for f in r[k][1:]]) for r in rounds] for k in range(3))
        for name, other in (("(half)", mh), ("(delta)", md)):
            verdicts.append(f"- {w}x{h}: medians per round, {name} {', '.join(f'{x:.4f}' for x in other)} ms; (delta half) {', '.join(f'{x:.4f}' for x in mdh)} ms: the "
                            f"half-block delta route is {'faster' if max(mdh) < min(other) else 'slower' if min(mdh) > max(other) else 'within the spread of the rounds'} "
                            f"({statistics.median(mdh) - statistics.median(other):+.4f} ms at the medians of the medians).")
        print()
        f0, f1 = o.frames_rgb8([0, 1])
        kernels.append((f"{w}x{h}, orbit frames 0 -> 1", kernel_times(o.ctx, f0, f1)))
        if (w, h) == SIZES[-1]:
            rng = np.random.default_rng(15)
            shown = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            nxt = shown ^ np.uint8(0x80)  # every cell changed; random colours: horizontal neighbours differ (but for one pair in 2^24)
            kernels.append((f"{w}x{h}, every cell changed, all neighbours different", kernel_times(o.ctx, shown, nxt)))
        o.close()
    print("## the three kernels (HIP events, median (min, max) of 20) beside text_from_rgb8_kernel<ansi_half_text> on the new frame (wall clock over 20 launches back to back)\n")
    print("| frames | delta text bytes | measure ms | offsets ms | write ms | sum ms | text_from_rgb8_kernel<ansi_half_text> ms (whole text) |")
    print("|---|---|---|---|---|---|---|")
    for what, (n, ms, whole) in kernels:
        total = [sum(x) for x in zip(*ms)]
        print(f"| {what} | {n} | {spread(ms[0])} | {spread(ms[1])} | {spread(ms[2])} | {spread(total)} | {whole:.4f} |")
    print("\n" + "\n".join(verdicts))


if __name__ == "__main__":
    main()
