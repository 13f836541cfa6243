#!/usr/bin/env python3
"""Generate tests/golden/camera_edges.npz and golden_camera_edges.json: the camera family of tests/support.py (camera_scenes) rendered
by the GENUINE reference's own project_scene, so that the three places where the kernels form a primary ray, and the host tables in
front of them, answer to the reference itself on cameras outside bench_camera()'s domain.

Like make_golden_edges.py it runs only where the reference exists, after `make -C oracle`:

    python tests/golden/make_golden_cameras.py

Every camera is rendered at the two shots of VALUE_SHOTS by the reference's -O3 build and by its -O1 build, each build in a child
process of its own: on a camera with a primary direction that is not finite or of zero length the reference indexes outside its
tables and dies.  A camera is recorded as a case only where both builds live and give the same bits at both shots; every other camera
is recorded BY NAME, with what happened, in the JSON's "undefined" list -- none is dropped silently.  The builder marks each camera
defined or not; an outcome that contradicts the mark ends the recipe.

What is written is data: the base scene's arrays, camera arrays, the reference's double framebuffers, hashes and counts.  Both files
are reproduced byte for byte by a second run.
"""
import concurrent.futures
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import support as T  # noqa: E402
from make_golden_edges import MAX_ARCHIVE_BYTES, MAX_NAN_SHARE, RefLib, RefLibO1, same_bits, write_archive  # noqa: E402

BUILDS = {"-O3": RefLib, "-O1": RefLibO1}
# the order in which frames of the first shot take their place in the archive while it stays within the bound: what the chain, batch
# and shard tests render first, then the rest as the builder lists them.  A case without a frame keeps its hash and counts; its tests
# take the positions of a difference from the oracle's frame.
FRAMES_FIRST = (T.CAMERA_BASE, T.CAMERA_WIDE) + T.CAMERA_TRIO


def child(index, build, path):
    """both shots of camera `index` by one build of the reference, into an archive at `path`"""
    _, scene, w, h, _ = T.camera_scenes()[index]
    with np.errstate(all="ignore"):
        frames = {f"b{b}_s{spp}": np.ascontiguousarray(BUILDS[build].get(b, spp).render(scene, w, h)) for b, spp in T.VALUE_SHOTS}
    np.savez(path, **frames)


def render_in_children(index, tmp):
    """{build: frames or what ended the child}"""
    out = {}
    for build in BUILDS:
        path = os.path.join(tmp, f"{index}{build}.npz")
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(index), build, path], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        if done.returncode == 0:
            out[build] = dict(np.load(path))
        elif done.returncode < 0:
            out[build] = f"the reference's {build} build ended with signal {-done.returncode}"
        else:
            raise SystemExit(f"camera {index}, {build}: the child failed with status {done.returncode}, which is not the reference's doing")
    return out


def stored_size(value):
    """what a member of the archive costs, near enough: its deflated bytes and the two headers that name it"""
    return len(zlib.compress(np.ascontiguousarray(value).tobytes(), 9)) + 400


def main():
    built = T.camera_scenes()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        outcomes = list(pool.map(lambda i: render_in_children(i, tmp), range(len(built))))
    arrays = {"scene": T.pack_scene(built[0][1])}
    cases, undefined, frames = [], [], {}
    for (name, scene, w, h, defined), got in zip(built, outcomes):
        assert np.array_equal(T.bits(T.pack_scene(scene))[:-15], T.bits(arrays["scene"])[:-15]), name  # one scene under every camera
        died = [v for v in got.values() if isinstance(v, str)]
        what = "; ".join(died)
        if not died:
            differ = [f"the reference's -O1 and -O3 builds differ in {int((T.bits(got['-O3'][k]) != T.bits(got['-O1'][k])).sum())} values at {k}"
                      for k in got["-O3"] if not same_bits(got["-O3"][k], got["-O1"][k])]
            what = "; ".join(differ)
        if bool(what) == defined:
            raise SystemExit(f"{name}: the builder marks it {'defined' if defined else 'undefined'}, but: {what or 'both builds live and agree'}")
        arrays["cam/" + name] = scene.camera
        if what:
            undefined.append({"name": name, "w": w, "h": h, "what": what})
            print(f"UNDEFINED {name}: {what}")
            continue
        for b, spp in T.VALUE_SHOTS:
            fb = got["-O3"][f"b{b}_s{spp}"]
            nans, infs = int(np.isnan(fb).sum()), int(np.isinf(fb).sum())
            if nans > MAX_NAN_SHARE * fb.size:
                raise SystemExit(f"{name}: {nans} of {fb.size} values are NaN, more than {MAX_NAN_SHARE:.0%}: a failure could hide among them")
            cases.append({"name": f"{name}/b{b}_s{spp}", "camera": name, "scene": "cam/" + name, "spheres": scene.num_spheres, "dir_lights": len(scene.dir_lights),
                          "point_lights": len(scene.point_lights), "w": w, "h": h, "b": b, "spp": spp,
                          "fb_fnv": T.fnv(T.canonical_nans(fb)), "nan": nans, "inf": infs, "distinct": int(np.unique(T.bits(fb)).size), "fb": None})
            if (b, spp) == T.VALUE_SHOTS[0]:
                frames[name] = fb
    # the frames of the first shot, as many as the bound leaves room for; a frame equal bit for bit to an earlier one is held once
    room = MAX_ARCHIVE_BYTES - sum(stored_size(v) for v in arrays.values()) - 4096
    held = {}
    by_camera = {c["camera"]: c for c in cases if (c["b"], c["spp"]) == T.VALUE_SHOTS[0]}
    for name in list(FRAMES_FIRST) + [n for n in frames if n not in FRAMES_FIRST]:
        fb = frames[name]
        at = held.get(fb.tobytes())
        if at is None:
            cost = stored_size(fb)
            if cost > room:
                continue
            room -= cost
            at = held[fb.tobytes()] = name + "/fb"
            arrays[at] = fb
        by_camera[name]["fb"] = at
    for c in cases:
        print(f"case {c['name']}: {c['w']}x{c['h']} fb={c['fb_fnv']} nan={c['nan']} inf={c['inf']} distinct={c['distinct']} frame: {c['fb'] or 'hash only'}")
    note = ("generated by tests/golden/make_golden_cameras.py from oracle/_ref (genuine reference, -O3; every case equal bit for bit to its -O1 "
            "build; each build ran in a child process).  fb_fnv: FNV-1a-64 of the double framebuffer with every NaN replaced by "
            "0x7ff8000000000000.  distinct: how many different 64-bit values the frame holds.  undefined: the cameras on which a build of the "
            "reference died or the two builds differ, with what happened; their camera arrays are in the archive, the library's own "
            "definitions judge them.  No camera was dropped.")
    path = os.path.join(HERE, "camera_edges.npz")
    write_archive(path, arrays)
    size = os.path.getsize(path)
    if size > MAX_ARCHIVE_BYTES:
        raise SystemExit(f"camera_edges.npz is {size} bytes, more than frames.npz ({MAX_ARCHIVE_BYTES})")
    with open(os.path.join(HERE, "golden_camera_edges.json"), "w") as fh:
        json.dump({"note": note, "cases": cases, "undefined": undefined}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {len(cases)} cases and {len(undefined)} undefined cameras, camera_edges.npz {size} bytes (bound {MAX_ARCHIVE_BYTES}), "
          f"{sum(c['fb'] is not None for c in cases)} cases with their frame")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), sys.argv[3], sys.argv[4])
    else:
        main()
