"""What the delta texts of a moving picture cost when the frames are rendered ahead in batches, for the demo scene on the reference's orbit
(60 cameras, t = k / 60) at 480x280 and at 1920x1080, 10 bounces, 10 rays per pixel, in both kinds of cell:

  (batch)   trt_render_host_batch_ansi_delta / trt_render_host_batch_ansi_delta_half, 8 cameras per call (the orbit's last call has 4):
            one render, three text kernels and two transfers per call (csrc/trt_ansi_delta_chain.h);
  (single)  trt_render_host_ansi_delta / trt_render_host_ansi_delta_half, one camera per call -- measured by tools/ansi_delta_bench.py and
            tools/ansi_delta_half_bench.py on a build of the PARENT commit, whose outputs this tool reads.

Two steps.  `--measure FILE.json` runs `--rounds` rounds on the GPU after one orbit of each kind to warm up and writes, per size, kind and
round, the host-to-host ms per frame of every call (call time / cameras) and its bytes, and the three chain kernels' durations by HIP events
(trt_ansi_delta_chain_kernel_times: the orbit's frame 0 shown, frames 1..8 the chain) beside the one-pair kernels' on frames 0 -> 1.  A
session takes the parent's two tools and this one in turn, a process each, several times.  `--report` then needs no GPU: it reads the
turns' JSON files (`--turns`) and the saved outputs of the parent's tools (`--baseline`, their "medians per round" lines) and writes the
markdown report (`--out`, profiles/r18/a_delta_batch.md holds one): both columns and their difference."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, SPP, FRAMES, BATCH = 10, 10, 60, 8
SIZES = ((480, 280), (1920, 1080))
KINDS = ("full", "half")


def spread(values, digits=4):
    return f"{statistics.median(values):.{digits}f} (min {min(values):.{digits}f}, max {max(values):.{digits}f})"


def measure(rounds):
    import numpy as np
    import torch
    from terminalraytracer_amd import hip
    from terminalraytracer_amd import scenes as S
    lib = hip.lib()
    entries = {"full": (lib.trt_render_host_batch_ansi_delta, hip.ansi_delta_capacity, hip.Context.ansi_delta_chain_kernel_times, hip.Context.ansi_delta_kernel_times),
               "half": (lib.trt_render_host_batch_ansi_delta_half, hip.ansi_delta_half_capacity, hip.Context.ansi_delta_half_chain_kernel_times,
                        hip.Context.ansi_delta_half_kernel_times)}
    out = {}
    for w, h in SIZES:
        ctx = hip.Context(0)
        cams = np.ascontiguousarray([S.orbit_camera(k / 60.0, w, h) for k in range(FRAMES)], dtype=np.float64)
        ctx.set_scene(S.demo_scene(S.synth_sky(256), cams[0]))
        rows = hip.RowSet.whole(w, h)
        text = np.zeros(BATCH * max(hip.ansi_delta_capacity(w, h), hip.ansi_delta_half_capacity(w, h)), dtype=np.uint8)  # the caller's buffer, reused
        lengths = (C.c_size_t * BATCH)()

        def orbit(kind):
            """per call: (cameras, bytes of their texts, host ms)"""
            ctx.ansi_delta_reset()  # every orbit starts with its keyframe
            calls = []
            for first in range(0, FRAMES, BATCH):
                n = min(BATCH, FRAMES - first)
                t0 = time.perf_counter()
                hip._check(entries[kind][0](ctx._h, cams[first:].ctypes.data, n, C.byref(rows), B, SPP, text.ctypes.data, text.size, lengths))
                calls.append((n, sum(lengths[:n]), (time.perf_counter() - t0) * 1e3))
            return calls

        for kind in KINDS:
            orbit(kind)
        result = {kind: {"rounds": []} for kind in KINDS}
        for _ in range(rounds):
            for kind in KINDS:
                result[kind]["rounds"].append(orbit(kind))
        # the kernels alone: frame 0 shown, frames 1..8 the chain; and the one pair 0 -> 1
        frames = np.stack([ctx.render_host_rgb8(cams[k], rows, B, SPP) for k in range(BATCH + 1)])
        d_frames = torch.from_numpy(frames.reshape(-1)).to("cuda:0")
        each = h * w * 3
        for kind in KINDS:
            _, capacity, chain_times, pair_times = entries[kind]
            room = torch.zeros(BATCH * capacity(w, h) + 8, dtype=torch.uint8, device="cuda:0")
            d_lengths = torch.zeros(BATCH, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            chain = (ctx, d_frames.data_ptr(), d_frames.data_ptr() + each, BATCH, w, h, room.data_ptr(), room.numel() - 8, d_lengths.data_ptr())
            pair = (ctx, d_frames.data_ptr(), d_frames.data_ptr() + each, w, h, room.data_ptr(), room.numel() - 8, d_lengths.data_ptr())
            for times, args, name in ((chain_times, chain, "chain_kernels"), (pair_times, pair, "pair_kernels")):
                for _ in range(3):
                    times(*args)
                ms = [times(*args) for _ in range(20)]
                result[kind][name] = [[m[k] for m in ms] for k in range(3)]
            chain_times(*chain)
            result[kind]["chain_bytes"] = int(d_lengths.sum().cpu())
        out[f"{w}x{h}"] = result
        ctx.close()
    return out


BASELINE = re.compile(r"^- (\d+x\d+): medians per round, \((full|half)\) [\d., ]+ ms; \((?:delta|delta half)\) ([\d., ]+) ms")


def report(turn_files, baseline_files, out):
    turns = [json.load(open(f)) for f in turn_files]
    single = {}  # (size, kind) -> the parent's medians per round, over all turns
    for f in baseline_files:
        for line in open(f):
            m = BASELINE.match(line)
            if m:
                single.setdefault((m.group(1), m.group(2)), []).extend(float(x) for x in m.group(3).split(","))
    lines = [f"# delta texts of the demo orbit rendered ahead in batches of {BATCH}: {FRAMES} cameras (t = k / 60), {B} bounces, {SPP} rays per pixel\n",
             "(batch) trt_render_host_batch_ansi_delta(_half), this tree; (single) trt_render_host_ansi_delta(_half) of the parent's build, by the parent's "
             f"tools/ansi_delta_bench.py and tools/ansi_delta_half_bench.py.  {len(turns)} turn(s) of one GPU session, the parent's two tools and this one a process "
             "each in every turn.  (batch) per round: host ms per frame = call time / cameras, median (min, max) over the calls behind the first (which holds "
             "the keyframe); (single) per round: the parent tools' median over the frames 1..59.\n",
             "| size | kind | (single) host ms per frame, medians per round | (batch) host ms per frame, per round | (batch) bytes per frame | (batch) first call, ms per frame | "
             "(batch) - (single) ms per frame, medians of the medians | verdict |", "|---|---|---|---|---|---|---|---|"]
    for size in (f"{w}x{h}" for w, h in SIZES):
        for kind in KINDS:
            rounds = [r for t in turns for r in t[size][kind]["rounds"]]
            per_round = [[ms / n for n, _, ms in r[1:]] for r in rounds]
            medians = [statistics.median(p) for p in per_round]
            bytes_per_frame = [b / n for r in rounds for n, b, _ in r[1:]]
            first = [r[0][2] / r[0][0] for r in rounds]
            base = single.get((size, kind), [])
            if base:
                verdict = "faster" if max(medians) < min(base) else "slower" if min(medians) > max(base) else "within the spread of the rounds"
                difference = f"{statistics.median(medians) - statistics.median(base):+.4f}"
            else:
                verdict, difference = "no baseline given", ""
            lines.append(f"| {size} | {kind} | {', '.join(f'{x:.4f}' for x in base)} | {'; '.join(spread(p) for p in per_round)} | {spread(bytes_per_frame, 0)} | "
                         f"{spread(first)} | {difference} | {verdict} |")
    lines += ["", "## the three chain kernels over 8 pairs of frames (orbit frame 0 shown, frames 1..8 the chain) beside the one-pair kernels on frames 0 -> 1 "
              "(HIP events, median (min, max) of 20 per turn, all turns together)\n",
              "| size | kind | chain bytes | chain measure ms | chain offsets ms | chain write ms | chain sum ms | chain sum / 8 | one pair: measure ms | offsets ms | write ms | sum ms |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for size in (f"{w}x{h}" for w, h in SIZES):
        for kind in KINDS:
            chain = [[x for t in turns for x in t[size][kind]["chain_kernels"][k]] for k in range(3)]
            pair = [[x for t in turns for x in t[size][kind]["pair_kernels"][k]] for k in range(3)]
            chain_sum, pair_sum = [sum(x) for x in zip(*chain)], [sum(x) for x in zip(*pair)]
            lines.append(f"| {size} | {kind} | {turns[0][size][kind]['chain_bytes']} | {spread(chain[0])} | {spread(chain[1])} | {spread(chain[2])} | {spread(chain_sum)} | "
                         f"{statistics.median(chain_sum) / BATCH:.4f} | {spread(pair[0])} | {spread(pair[1])} | {spread(pair[2])} | {spread(pair_sum)} |")
    text = "\n".join(lines) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", metavar="FILE.json", help="run on the GPU and write the figures of this turn")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--report", action="store_true", help="write the markdown report of the turns; needs no GPU")
    ap.add_argument("--turns", nargs="*", default=[], help="the JSON files of --measure")
    ap.add_argument("--baseline", nargs="*", default=[], help="saved outputs of the parent's tools/ansi_delta_bench.py and tools/ansi_delta_half_bench.py")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r18", "a_delta_batch.md"))
    args = ap.parse_args()
    if args.measure:
        with open(args.measure, "w") as f:
            json.dump(measure(args.rounds), f)
    if args.report:
        report(args.turns, args.baseline, args.out)


if __name__ == "__main__":
    main()
