#!/usr/bin/env python3
"""Device time per frame of the 60-camera orbit at 1920x1080, BASELINE configs 3 and 5, three ways:

  single     one frame at a time on one context (trt_render_device, synchronised after every frame)
  pipelined  three frames in flight through trt_dist_* (what bench.py --animation does)
  batch n    trt_render_device_batch, n = 2, 4, 8 cameras per call, one call at a time

Times come from the library's events (trt_render_kernel_times, trt_launch_span_ms): the span from the start of the first launch
of a pass to the end of its last, divided by the frames.  Every way is repeated --reps times, the ways interleaved; the table shows
mean and min..max over the repetitions.  The last frame of every batch pass (camera 59) is hashed against golden_full.json.

    python tools/batch_bench.py [--configs c3,c5] [--reps 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import support as T  # noqa: E402
from terminalraytracer_amd import hip, host  # noqa: E402

W, H, FRAMES = 1920, 1080, 60
CONFIGS = {"c3": "c3_1080p_64sph_b8_f59", "c5": "c5_1080p_256sph_b12_f59"}


def orbit():
    cams = np.load(os.path.join(T.GOLDEN, "cameras_anim.npz"))["camera"][:FRAMES].copy()
    cams[:, 13] = 5.0 * W / H
    return cams


def span_per_frame(ctx, first_launch, frames):
    return ctx.launch_span_ms(first_launch, ctx, ctx.launch_count() - 1) / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    cams, rows = orbit(), hip.RowSet.whole(W, H)
    result = {}
    for name in args.configs.split(","):
        case = T.golden_full()[CONFIGS[name]]
        scene = T.full_scene(case)
        b, spp = case["bounce_limit"], case["rays_per_pixel"]
        assert np.array_equal(np.array(case["camera"]), cams[59]), "the stored orbit ends on the golden's camera"
        fb = torch.zeros(8 * H * W * 3, dtype=torch.float64, device="cuda:0")
        ways = {"single": [], "pipelined": [], "batch 2": [], "batch 4": [], "batch 8": []}
        info, ok = {}, True
        with hip.Context(0) as ctx:
            ctx.set_scene(scene)
            d = hip.Dist(0, scene, None, 0, 1, W, H, frames_in_flight=3)
            try:
                for rep in range(args.reps + 1):  # the first repetition warms everything up and is dropped
                    took = {}
                    first = ctx.launch_count()
                    for cam in cams:
                        ctx.render_device(cam, rows, b, spp, fb.data_ptr(), H * W * 24)
                        ctx.synchronize()
                    took["single"] = float(np.sum(ctx.kernel_times(FRAMES))) / FRAMES
                    slots = [d.context(k) for k in range(3)]
                    before = [c.launch_count() for c in slots]
                    for cam in cams:
                        d.render(cam, b, spp)
                    d.synchronize()
                    took["pipelined"] = max(c0.launch_span_ms(a0, c1, c1.launch_count() - 1) for c0, a0 in zip(slots, before) for c1 in slots) / FRAMES
                    for n in (2, 4, 8):
                        first = ctx.launch_count()
                        for at in range(0, FRAMES, n):
                            part = cams[at:at + n]
                            ctx.render_device_batch(part, rows, b, spp, fb.data_ptr(), fb.numel() * 8)
                            if at == 0:  # a full batch of n: (frames, render launches) and the form it ran
                                info[f"batch {n}"] = {"frames_launches": ctx.batch_info(), "decoupled": ctx.render_variant()["decoupled"]}
                        ctx.synchronize()
                        took[f"batch {n}"] = span_per_frame(ctx, first, FRAMES)
                        last = len(part) - 1
                        frame = fb[last * H * W * 3:(last + 1) * H * W * 3].cpu().numpy()
                        ok = ok and host.fnv1a64(frame) == case["fb_fnv"]
                    if rep:
                        for k, v in took.items():
                            ways[k].append(v)
            finally:
                d.close()
        result[name] = {"frames": FRAMES, "reps": args.reps, "last_frame_matches_reference": ok, "batch_calls": info,
                        "ms_per_frame": {k: {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in ways.items()}}
        print(f"{name}: {case['spheres']} spheres, {b} bounces, {spp} rays per pixel, {FRAMES} cameras, {args.reps} repetitions; last frames match the reference: {ok}")
        for k, v in result[name]["ms_per_frame"].items():
            print(f"  {k:10s} {v['mean']:.3f} ms/frame  ({v['min']:.3f} .. {v['max']:.3f})  {info.get(k, '')}")
        del fb
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0 if all(r["last_frame_matches_reference"] for r in result.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
