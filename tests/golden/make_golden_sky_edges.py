#!/usr/bin/env python3
"""The GENUINE reference's texel for every direction of tests/sky_edges.py (oracle/_ref, built by oracle/Makefile from
/root/reference/TerminalRayTracer.c where it lies).

    python tests/golden/make_golden_sky_edges.py        # build container only

For each cubemap side of sky_edges.SIDES the reference's own get_skybox_color (TerminalRayTracer.c:700) looks every direction up
in an INDEX-CODED sky: a texel's RGB is its number, r + 256 g + 65536 b.  Up to 256 texels a side that number is
face * dim^2 + index; above, two skies are used, one coding the index within the face and one the face, and the reference is
called on each.  The skies are generated here and not kept.

The reference reads outside the face's table where u_index + v_index * dim is not below dim^2 (u == 0.5 in the last row): there
it is not defined, trt_oracle_skybox_lookup says so, the reference is not called and -1 is recorded.  Everywhere else both the
-O3 and the -O1 build are asked, and the number is recorded only where they agree (-2 otherwise; the run reports how many: none).
normalize_vector (:439) is held against sky_edges.normalised on the way, bit for bit.

Writes sky_edges.npz -- per side the int32 texel numbers, nothing else: the directions are rebuilt by whoever reads it -- and
sky_edges.json: per side the FNV-1a-64 of the directions' bytes and of the numpy-normalised directions' bytes, the counts of the
classes the rational model of sky_edges.py sorts the directions into, and how many in-face look-ups are decided by rounding alone
(the real-arithmetic index is not the reference's).  Both files come out byte for byte on a second run."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import sky_edges as E  # noqa: E402
import support as T  # noqa: E402
from make_golden import RefLib  # noqa: E402
from make_golden_edges import RefLibO1, write_archive  # noqa: E402

MAX_ARCHIVE_BYTES = os.path.getsize(os.path.join(HERE, "frames.npz"))
VARIANT = (4, 10)  # any variant with an -O1 twin: get_skybox_color reads none of the build's macros


def reference_numbers(lib, scene_data, dirs, ask):
    """r + 256 g + 65536 b of get_skybox_color's texel for the directions with `ask`"""
    scene = scene_data.as_scene()
    out = np.full(len(dirs), -1, dtype=np.int64)
    for i in np.nonzero(ask)[0]:
        d = T.L.Vector(*dirs[i])
        col = T.L.Color()
        lib.get_skybox_color(C.byref(scene), C.byref(d), C.byref(col))
        out[i] = col.r + 256 * col.g + 65536 * col.b
    return out


def main():
    refs = [RefLib.get(*VARIANT), RefLibO1.get(*VARIANT)]
    for r in refs:
        r.lib.normalize_vector.argtypes = [C.POINTER(T.L.Vector)]
    arrays, meta = {}, {}
    for dim in E.SIDES:
        dirs, _ = E.directions(dim)
        unit = E.normalised(dirs)
        for i in range(0, len(dirs), 7):  # the numpy normalisation is the reference's
            v = T.L.Vector(*dirs[i])
            refs[0].lib.normalize_vector(C.byref(v))
            assert np.array_equal(np.array([v.x, v.y, v.z]).view(np.uint64), unit[i].view(np.uint64)), (dim, i)
        face, index, inside = E.oracle_lookup(T.oracle(), dim, dirs)
        if dim <= 256:
            numbers = [reference_numbers(r.lib, E.coded_scene(dim), dirs, inside) for r in refs]
        else:
            numbers = []
            for r in refs:
                within = reference_numbers(r.lib, E.coded_scene(dim, "index"), dirs, inside)
                which = reference_numbers(r.lib, E.coded_scene(dim, "face"), dirs, inside)
                numbers.append(np.where(inside, which * dim * dim + within, -1))
        agree = numbers[0] == numbers[1]
        texel = np.where(inside, np.where(agree, numbers[0], -2), -1).astype(np.int32)
        m = E.model(dim)
        recorded = texel >= 0
        rounding = recorded & (m["face"] * dim * dim + m["index"] != texel)
        per_face = [[int(((m["cls"] == c) & (m["face"] == f)).sum()) for c in range(4)] for f in range(6)]
        meta[str(dim)] = {
            "directions": int(len(dirs)), "dirs_fnv": T.fnv(dirs), "unit_fnv": T.fnv(unit),
            "outside": int((texel == -1).sum()), "builds_disagree": int((texel == -2).sum()), "recorded": int(recorded.sum()),
            "classes": {name: int((m["cls"] == c).sum()) for c, name in enumerate(E.CLASS_NAMES)},
            "classes_per_face": per_face,
            "decided_by_rounding": int(rounding.sum()),
            "decided_by_rounding_per_face": [int((rounding & (texel // (dim * dim) == f)).sum()) for f in range(6)],
            "decided_by_rounding_share": round(float(rounding.sum()) / float(recorded.sum()), 4),
        }
        arrays[f"texel_{dim}"] = texel
        print(dim, json.dumps(meta[str(dim)]))
        assert (face * dim * dim + index)[recorded].tolist() == texel[recorded].tolist(), "the oracle differs from the reference"
    path = os.path.join(HERE, "sky_edges.npz")
    write_archive(path, arrays)
    size = os.path.getsize(path)
    assert size <= MAX_ARCHIVE_BYTES, (size, MAX_ARCHIVE_BYTES)
    note = ("generated by tests/golden/make_golden_sky_edges.py from oracle/_ref (genuine reference, get_skybox_color at -O3 and -O1) for "
            "the directions of tests/sky_edges.py.  texel_<dim>: face * dim^2 + index, -1 where the reference reads outside the face.  "
            "classes: what the rational model of tests/sky_edges.py says of the directions; decided_by_rounding: recorded look-ups whose "
            "real-arithmetic index is not the reference's.")
    with open(os.path.join(HERE, "sky_edges.json"), "w") as fh:
        json.dump({"note": note, "archive_bytes": size, "sides": meta}, fh, indent=1)
        fh.write("\n")
    print("wrote sky_edges.npz", size, "bytes")


if __name__ == "__main__":
    main()
