#!/usr/bin/env python3
"""Library builds in turn through the tools that time the whole-frame output kinds (TRT_HIP_LIB selects the build): ansi_path_bench,
ansi_half_bench, ansi256_bench, kitty_bench, sixel_bench and ansi_delta_bench, a process each, the order of the builds rotating from turn
to turn.  Every tool's report is kept under --out; the table printed at the end lists every millisecond figure of a row of the size
asked for -- a figure per turn is the median the tool prints -- with the FIRST build's min .. max over the turns as the yardstick for
the medians of the others.  --parse: only read the reports of an earlier run.

usage: python3 tools/output_kinds_ab.py [--turns 3] [--size 1920x1080] [--out build/output_kinds] build/parent.so terminalraytracer_amd/libtrt_hip.so
"""
import argparse
import collections
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TOOLS = (("ansi_path_bench", ["--rounds", "3"]), ("ansi_half_bench", ["--rounds", "3"]), ("ansi256_bench", ["--rounds", "3"]),
         ("kitty_bench", ["--rounds", "3"]), ("sixel_bench", ["--rounds", "1"]), ("ansi_delta_bench", ["--rounds", "1"]))
NUMBER = re.compile(r"^\s*(\d+\.\d+)")


def figures(report, size):
    """{figure: ms} of the markdown tables of a tool's report: the cells that start with a decimal number, in rows that name the size, or
    name none under a line that does, and in columns that count neither bytes nor colours; a figure is named by the start of the line in
    front of its table, its row's labels and its column"""
    out, header, title, last = {}, None, "", ""
    for line in report.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")] if line.startswith("|") else None
        if cells is None:
            header, last = None, line.strip() or last
        elif header is None:
            header, title = cells, last.lstrip("# ")[:48]
        elif not set(line) <= set("|-: ") and (any(size in c for c in cells) or (size in title and not re.match(r"\d+x\d+", cells[0]))):
            labels = [c for c in cells[:3] if not re.match(r"\d+(\.\d+)?( \(|$)", c)]
            for name, cell in zip(header, cells):
                m = NUMBER.match(cell)
                if m and "bytes" not in name and "colours" not in name:
                    out[", ".join([title, *labels, name])] = float(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default="build/output_kinds")
    ap.add_argument("--budget", type=float, default=900, help="seconds after which no further turn is started")
    ap.add_argument("--parse", action="store_true")
    ap.add_argument("libs", nargs="+")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    path = lambda turn, k, tool: os.path.join(args.out, f"turn{turn}_lib{k}_{tool}.md")
    t0, turns = time.time(), 0
    for turn in range(args.turns):
        if args.parse or time.time() - t0 > args.budget:
            break
        for k in [(turn + i) % len(args.libs) for i in range(len(args.libs))]:
            for tool, options in TOOLS:
                env = dict(os.environ, TRT_HIP_LIB=os.path.abspath(args.libs[k]))
                done = subprocess.run([sys.executable, os.path.join(HERE, tool + ".py"), *options], env=env, capture_output=True, text=True, timeout=240)
                if done.returncode:  # nothing more is started on the GPU behind a tool that failed
                    sys.exit(f"{tool} with {args.libs[k]} ended with {done.returncode}:\n{done.stderr[-2000:]}")
                with open(path(turn, k, tool), "w") as fh:
                    fh.write(done.stdout)
        turns += 1
        print(f"turn {turn} done after {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
    if args.parse:
        turns = sum(os.path.exists(path(t, 0, TOOLS[0][0])) and os.path.exists(path(t, len(args.libs) - 1, TOOLS[-1][0])) for t in range(args.turns))
    table = collections.defaultdict(lambda: [[] for _ in args.libs])
    for turn in range(turns):
        for k in range(len(args.libs)):
            for tool, _ in TOOLS:
                with open(path(turn, k, tool)) as fh:
                    for figure, ms in figures(fh.read(), args.size).items():
                        table[(tool, figure)][k].append(ms)
    others = "".join(f" {lib}, per turn | median | |" for lib in args.libs[1:])
    print(f"{turns} turns; the yardstick is the min .. max of `{args.libs[0]}` over its turns.\n")
    print(f"| tool | figure | {args.libs[0]}, per turn | min .. max |{others}")
    print("|---|---|---|---|" + "---|---|---|" * (len(args.libs) - 1))
    for (tool, figure), per_lib in sorted(table.items()):
        lo, hi = min(per_lib[0]), max(per_lib[0])
        row = f"| `{tool}` | {figure} | {', '.join(f'{x:.4f}' for x in per_lib[0])} | {lo:.4f} .. {hi:.4f} |"
        for ms in per_lib[1:]:
            med = statistics.median(ms)
            row += f" {', '.join(f'{x:.4f}' for x in ms)} | {med:.4f} | {'ABOVE (slower)' if med > hi else 'below (faster)' if med < lo else 'within'} |"
        print(row)


if __name__ == "__main__":
    main()
