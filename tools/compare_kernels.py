#!/usr/bin/env python3
"""Are the kernels of one build of the library the kernels of another?  No GPU is needed.

usage: tools/compare_kernels.py OLD.s NEW.s [--dropped-parameter KERNEL=POSITION ...]

OLD.s and NEW.s are the device assembly of one translation unit from two trees, e.g.
    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -o NEW.s terminalraytracer_amd/csrc/trt_render.hip
For every kernel of OLD the instructions, the kernel descriptor (.amdhsa_*: registers, LDS, scratch) and the resource notes the
compiler prints behind the body must be the same text in NEW; the kernels NEW has beyond those are listed with their resources.

A template parameter added at the end of a kernel's list changes every mangled name of that kernel.  --dropped-parameter
render_rounds_kernel=8 says: in NEW, a render_rounds_kernel whose boolean template argument 8 (counted from 0) is false is OLD's kernel
without that argument; one whose argument is true is new."""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    """{mangled name: the kernel's text -- instructions, descriptor, the compiler's resource notes -- with compiler-numbered labels and
    the kernel's own name made neutral}"""
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M):
        chunk = re.search(r"^%s:.*?^; Kernel info:\n(?:;[^\n]*\n)+" % re.escape(name), text, flags=re.M | re.S).group(0)
        chunk = re.sub(r"\.L(func_end|tmp)\d+", r".L\1", chunk.replace(name, "KERNEL"))
        out[name] = re.sub(r"BB\d+_", "BB_", chunk)  # the function's number in the unit, in labels and in the loop comments
    return out


def resources(chunk):
    get = lambda key: (re.search(r"^; " + key + r":\s*(\d+)", chunk, flags=re.M) or [None, "?"])[1]  # noqa: E731
    return {"vgprs": get("NumVgprs"), "agprs": get("NumAgprs"), "sgprs": get("TotalNumSgprs"), "scratch": get("ScratchSize"),
            "lds": get("LDSByteSize"), "waves": get("Occupancy")}


def main(argv):
    old_path, new_path = argv[1], argv[2]
    dropped = {}
    for a in argv[3:]:
        if a == "--dropped-parameter":
            continue
        k, pos = a.split("=")
        dropped[k] = int(pos)
    old, new = kernels(old_path), kernels(new_path)
    old_names, new_names = demangle(list(old)), demangle(list(new))

    def as_old(pretty):
        """the demangled name the kernel had before the parameter was added, or None if the argument is not false"""
        m = re.match(r"(void )?(\w+::)*(\w+)<(.*?)>\(", pretty)
        if not m or m.group(3) not in dropped:
            return pretty
        args = m.group(4).split(", ")
        pos = dropped[m.group(3)]
        if pos >= len(args):
            return pretty
        if args[pos] != "false":
            return None
        del args[pos]
        return pretty[: m.start(4)] + ", ".join(args) + pretty[m.end(4):]

    by_old_name = {}
    fresh = []
    for mangled, pretty in new_names.items():
        was = as_old(pretty)
        if was is None:
            fresh.append(mangled)
        else:
            by_old_name[was] = mangled
    differ = missing = 0
    for mangled, pretty in old_names.items():
        twin = by_old_name.pop(pretty, None)
        if twin is None:
            print("MISSING in new:", pretty)
            missing += 1
            continue
        same = old[mangled] == new[twin]
        r = resources(old[mangled])
        print("%s  %s  %s" % ("same  " if same else "DIFFER", " ".join("%s=%s" % kv for kv in r.items()), pretty.split("(")[0]))
        if not same:
            differ += 1
            print("    %d against %d lines; now" % (old[mangled].count("\n"), new[twin].count("\n")), resources(new[twin]))
    fresh += list(by_old_name.values())
    for mangled in fresh:
        r = resources(new[mangled])
        print("NEW     %s  %s" % (" ".join("%s=%s" % kv for kv in r.items()), new_names[mangled].split("(")[0]))
    print("%d kernels of the old build: %d differ, %d missing; %d new" % (len(old), differ, missing, len(fresh)))
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
