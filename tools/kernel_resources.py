"""Per-kernel VGPR / AGPR / LDS / scratch of a built gfx950 library (the code
object metadata tests/test_codeobject.py checks), filtered by a regex.

usage: python tools/kernel_resources.py [regex] [--lib path/to/lib.so] [--against path/to/other.so]

--against OTHER_LIB prints no table: it lists the kernels (of the regex) that only one of the two
libraries has, whose figures differ, or whose code bytes differ, and ends with a count.  It compares
metadata and bytes only; it inspects no instruction.  Either path may be one object file of a build.
"""
import argparse
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def _tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_objects(lib, d):
    """The gfx950 code objects of lib's fat binary, written under d: their paths."""
    fat = os.path.join(d, "fatbin.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib,
                    os.path.join(d, "lib.stripped")], check=True)
    blob = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    out = []
    for i, st in enumerate(starts):
        part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"b{i}.o")
        with open(part, "wb") as f:
            f.write(blob[st:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        out.append(co)
    return out


def notes_of(co):
    out = {}
    for ent in re.split(r"\n\s+- \.agpr_count:", _tool("llvm-readelf", "--notes", co))[1:]:
        field = lambda k: re.search(rf"\.{k}:\s+(\S+)", ent)  # noqa: E731
        if field("name") is None or field("vgpr_count") is None:
            continue
        out[field("name").group(1)] = (int(field("vgpr_count").group(1)), int(ent.split("\n", 1)[0].strip()),
                                       int(field("group_segment_fixed_size").group(1)),
                                       int(field("private_segment_fixed_size").group(1)))
    return out


def code_of(co):
    """name -> the bytes of every function symbol of code object co."""
    blob = open(co, "rb").read()
    sections = {}  # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", _tool("llvm-readelf", "-S", "-W", co), re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    out = {}
    for line in _tool("llvm-readelf", "-s", "-W", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6].isdigit():
            addr, off = sections[int(f[6])]
            start = int(f[1], 16) - addr + off
            out[f[7]] = blob[start:start + int(f[2])]
    return out


def kernel_notes(lib):
    with tempfile.TemporaryDirectory() as d:
        out = {}
        for co in code_objects(lib, d):
            out.update(notes_of(co))
    return out


def kernels(lib):
    """name -> ((vgpr, agpr, lds, scratch), code bytes) of every kernel of lib."""
    with tempfile.TemporaryDirectory() as d:
        out = {}
        for co in code_objects(lib, d):
            code = code_of(co)
            out.update({name: (fig, code.get(name)) for name, fig in notes_of(co).items()})
    return out


def compare(lib, other, pattern):
    a, b = ({k: v for k, v in kernels(p).items() if re.search(pattern, k)} for p in (lib, other))
    differ = 0
    for name in sorted(a.keys() | b.keys()):
        if name not in a or name not in b:
            what = f"only in {other if name in b else lib}"
        elif a[name][0] != b[name][0]:
            what = "figures " + " -> ".join("vgpr %d agpr %d lds %d scratch %d" % x[name][0] for x in (b, a))
        elif a[name][1] != b[name][1]:
            what = f"code bytes differ ({len(b[name][1])} -> {len(a[name][1])})"
        else:
            continue
        differ += 1
        print(f"{name}: {what}")
    print(f"{differ} of {len(a.keys() | b.keys())} kernels differ ({len(a)} in {lib}, {len(b)} in {other})")
    return differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pattern", nargs="?", default=".")
    ap.add_argument("--lib", default=os.path.join(REPO, "quantized-kv-cache-ecc-protection_amd", "kvecc", "libkvecc.so"))
    ap.add_argument("--against", metavar="OTHER_LIB", help="list the kernels that differ from OTHER_LIB's (figures, code bytes)")
    args = ap.parse_args()
    if args.against:
        raise SystemExit(1 if compare(args.lib, args.against, args.pattern) else 0)
    for name, (v, a, lds, scr) in sorted(kernel_notes(args.lib).items()):
        if re.search(args.pattern, name):
            print(f"vgpr {v:3d} agpr {a:3d} lds {lds:6d} scratch {scr:4d}  {name}")


if __name__ == "__main__":
    main()
