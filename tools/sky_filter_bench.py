"""What bilinear sky filtering (trt_set_sky_filter) costs on the device: render-kernel ms (trt_render_kernel_times) per 1920x1080 frame of
BASELINE configs 2, 3 and 5 (bench.py's workloads c2, c3, c5; 10 rays per pixel, the stored camera of orbit time 1.0), filter on
against off, in one build.  Config 3 with the filter on leaves the decoupled kernel for the plain rounds, so every config is also
measured at trt_set_compaction(0): on against off there is the filter's own cost, the rest is the lost decoupling; the row at
trt_set_compaction(-1) is the whole price of switching on.  Also: registers and workgroups per CU of the four filtering
instantiations beside their plain twins (trt_kernel_info), and two PPMs of the reference's demo scene, filter on and off (--ppm DIR).

Every step that uses the GPU is a child process of its own under its own time limit; the first step that fails ends the run.  Prints a
markdown report (profiles/r28/a_sky_filter.md holds one)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPP = 10
STEP_SECONDS = 240


def spread(values):
    return f"{statistics.median(values):.3f} (min {min(values):.3f}, max {max(values):.3f})"


def render_ms(ctx, hip, scene, w, h, bounces, frames):
    rows = hip.RowSet.whole(w, h)
    for _ in range(frames):
        ctx.render_host_rgb8(scene.camera, rows, bounces, SPP)
    return statistics.median(ctx.render_kernel_times(frames)[0])


def step_config(workload, compaction, rounds, frames):
    import bench
    from terminalraytracer_amd import hip
    w = bench.WORKLOADS[workload]
    scene = bench.build_scene(workload)
    out = {"workload": workload, "compaction": compaction, "off": [], "on": [], "variant": {}}
    with hip.Context(0) as ctx:
        ctx.set_compaction(compaction)
        ctx.set_scene(scene)
        for on in (0, 1):  # warm both
            ctx.set_sky_filter(on)
            render_ms(ctx, hip, scene, w["width"], w["height"], w["bounces"], 3)
            out["variant"]["on" if on else "off"] = dict(ctx.render_variant(), **ctx.kernel_info())
        for _ in range(rounds):  # the two take turns
            for on in (0, 1):
                ctx.set_sky_filter(on)
                out["on" if on else "off"].append(render_ms(ctx, hip, scene, w["width"], w["height"], w["bounces"], frames))
    print(json.dumps(out))


def step_kernels():
    """registers and workgroups per CU of the four filtering instantiations and their plain twins, on a 64-sphere scene"""
    import bench
    from terminalraytracer_amd import hip
    scene = bench.build_scene("c3")
    rows = hip.RowSet.whole(64, 36)
    out = []
    with hip.Context(0) as ctx:
        ctx.set_compaction(0)
        for m in (0, 2):
            ctx.set_path_patches(m)
            ctx.set_scene(scene)
            for count in (False, True):
                ctx.enable_counters(count)
                for on in (0, 1):
                    ctx.set_sky_filter(on)
                    ctx.render_host(scene.camera, rows, 4, 3)
                    out.append(dict(patches=m, counters=count, sky_filter=on, **ctx.kernel_info()))
    print(json.dumps(out))


def step_ppm(directory):
    from terminalraytracer_amd import hip
    from terminalraytracer_amd import scenes as S
    w, h = 320, 180
    scene = S.demo_scene(S.synth_sky(256), S.orbit_camera(1.0, w, h))
    os.makedirs(directory, exist_ok=True)
    frames = {}
    with hip.Context(0) as ctx:
        ctx.set_scene(scene)
        for name, mode in (("on", 1), ("off", 0)):
            ctx.set_sky_filter(mode)
            frames[name] = ctx.render_host_rgb8(scene.camera, hip.RowSet.whole(w, h), 10, SPP)
            with open(os.path.join(directory, f"a_sky_filter_{name}_320x180.ppm"), "wb") as fh:
                fh.write(b"P6\n%d %d\n255\n" % (w, h) + frames[name].tobytes())
    changed = int((frames["on"] != frames["off"]).any(axis=2).sum())
    step = int(abs(frames["on"].astype(int) - frames["off"].astype(int)).max())
    print(json.dumps({"directory": directory, "changed_pixels": changed, "pixels": w * h, "largest_byte_step": step}))


def child(*step):
    """one GPU step as a process of its own, under its own time limit; its last line is its JSON result"""
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", *[str(s) for s in step]], capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
    if run.returncode != 0:
        sys.exit(f"step {step} ended with status {run.returncode}; nothing further is started\n{run.stderr[-2000:]}")
    return json.loads(run.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20, help="frames per round and setting; a cell is the median of the rounds' medians")
    ap.add_argument("--ppm", metavar="DIR", help="write the demo scene with the filter on and off as PPM files there")
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        kind = args.step[0]
        if kind == "config":
            step_config(args.step[1], int(args.step[2]), int(args.step[3]), int(args.step[4]))
        elif kind == "kernels":
            step_kernels()
        else:
            step_ppm(args.step[1])
        return
    print(f"# bilinear sky filtering on the device: render-kernel ms per 1920x1080 frame, {SPP} rays per pixel\n")
    print(f"{args.rounds} rounds of {args.frames} frames per setting, off and on taking turns; a cell is the median over the rounds (min, max) of a round's median.\n")
    print("| config | trt_set_compaction | off: kernel | off, ms | on: kernel | on, ms | on / off |")
    print("|---|---|---|---|---|---|---|")
    for workload in ("c2", "c3", "c5"):
        for compaction in (-1, 0):
            r = child("config", workload, compaction, args.rounds, args.frames)
            kernel = {k: f"{'decoupled' if v['decoupled'] else 'plain rounds'}, {v['workgroup_threads']} threads, {v['vgprs']} VGPRs, {v['max_blocks_per_cu']} workgroups/CU"
                      for k, v in r["variant"].items()}
            ratio = statistics.median(r["on"]) / statistics.median(r["off"])
            print(f"| {workload} | {compaction} | {kernel['off']} | {spread(r['off'])} | {kernel['on']} | {spread(r['on'])} | {ratio:.3f} |", flush=True)
    print("\nThe four filtering instantiations beside their twins (trt_kernel_info after a launch of each; 512 VGPRs a SIMD: up to 128 is four waves, "
          "up to 168 three):\n")
    print("| patches m | counters | sky filter | VGPRs | workgroups per CU the launch is sized by |")
    print("|---|---|---|---|---|")
    for k in child("kernels"):
        over = "  (more than 128: three waves a SIMD)" if k["vgprs"] > 128 else ""
        print(f"| {k['patches']} | {'on' if k['counters'] else 'off'} | {'on' if k['sky_filter'] else 'off'} | {k['vgprs']}{over} | {k['max_blocks_per_cu']} |")
    if args.ppm:
        r = child("ppm", args.ppm)
        print(f"\nThe reference's demo scene (orbit time 1.0, 10 bounces, a 256^2 synthetic sky) at 320x180 with the filter on and off: a_sky_filter_on_320x180.ppm, "
              f"a_sky_filter_off_320x180.ppm; {r['changed_pixels']} of {r['pixels']} pixels differ in their bytes, by at most {r['largest_byte_step']} of 255.")


if __name__ == "__main__":
    main()
